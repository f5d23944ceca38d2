"""The batched FOV ingest and KittiDataset without a GPU: the agreement of include/dfu3d_ingest.h with its binding,
argument validation before any launch, the NumPy restatement against golden G18 (the reference's own get_fov_flag,
boxes3d_kitti_camera_to_lidar, get_infos and in_hull counts), and the dataset's host logic on a temporary KITTI
directory."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from dfu3d_amd import _build, _lib, _lib_ingest
from tests import ingest_cases as K
from tests import ingest_ref as R

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch


@pytest.fixture(scope="module")
def G():
    return K.golden()


def test_header_and_binding_agree():
    assert _lib_ingest.HEADER == os.path.join(_build.INCLUDE, "dfu3d_ingest.h") and _lib_ingest.HEADER in _build._deps()
    assert _lib_ingest.header_symbols() == ['dfu3d_fov_ingest', 'dfu3d_fov_ingest_scratch_bytes', 'dfu3d_ing_version']
    L = _lib_ingest.lib()                                               # raises naming every symbol the library lacks
    assert all(hasattr(L, s) for s in _lib_ingest.header_symbols())
    assert L.dfu3d_ing_version() == _lib_ingest.header_version() == 1
    C = _lib_ingest.CONSTANTS
    assert all(k.startswith("DFU3D_ING_") for k in C)
    assert C['DFU3D_ING_LAUNCHES'] == 4 and C['DFU3D_ING_CHUNK'] % 64 == 0
    assert (C['DFU3D_ING_EMIT'], C['DFU3D_ING_COUNT'], C['DFU3D_ING_ST_OFFSETS'], C['DFU3D_ING_ST_SHAPE']) == (1, 2, 1, 2)
    res, args = _lib_ingest.SIGNATURES['dfu3d_fov_ingest']
    assert res is ctypes.c_int32 and len(args) == 18 and args[15] is ctypes.c_size_t
    assert _lib_ingest.SIGNATURES['dfu3d_fov_ingest_scratch_bytes'] == (ctypes.c_size_t, [ctypes.c_int64])
    assert not set(_lib_ingest.SIGNATURES) & set(_lib.SIGNATURES) and len(_lib.SIGNATURES) == 46
    for other in ("dfu3d.h", "dfu3d_vfe.h", "dfu3d_head.h", "dfu3d_post.h", "dfu3d_aug.h", "dfu3d_bev.h", "dfu3d_opt.h"):
        assert "dfu3d_ing" not in open(os.path.join(_build.INCLUDE, other)).read()
    from dfu3d_amd import ingest_ops
    assert (ingest_ops.EMIT, ingest_ops.COUNT, ingest_ops.LAUNCHES, ingest_ops.CALIB_FLOATS) == (1, 2, 4, 48)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
        dfu3d_ing_version = object()
    with pytest.raises(_lib.Dfu3dError, match="dfu3d_fov_ingest, dfu3d_fov_ingest_scratch_bytes"):
        _lib_ingest.bind(Fake())


def _call(L, points=P16, n_rows=10, C=4, point_off=P16, B=2, calib=P16, shape=P16, boxes=P16, n_boxes=3, box_off=P16, mode=3,
          out=ctypes.c_void_p(32), out_off=P16, box_cnt=P16, scratch=P16, scratch_bytes=1 << 20, status=P16):
    return L.dfu3d_fov_ingest(points, n_rows, C, point_off, B, calib, shape, boxes, n_boxes, box_off, mode, out, out_off,
                              box_cnt, scratch, scratch_bytes, status, None)


def test_bad_arguments_return_before_any_launch():
    L = _lib_ingest.lib()
    EINVAL, ERANGE = _lib.CONSTANTS["DFU3D_EINVAL"], _lib.CONSTANTS["DFU3D_ERANGE"]
    C = _lib_ingest.CONSTANTS
    odd = ctypes.c_void_p(18)
    bad = [dict(B=0), dict(B=-1), dict(n_rows=-1), dict(C=2), dict(n_boxes=-1), dict(mode=0), dict(mode=4), dict(mode=7),
           dict(point_off=None), dict(calib=None), dict(shape=None), dict(status=None), dict(scratch=None),
           dict(points=None), dict(out=None), dict(out=P16), dict(out_off=None), dict(box_off=None), dict(boxes=None),
           dict(box_cnt=None), dict(point_off=ctypes.c_void_p(20)), dict(scratch=ctypes.c_void_p(20)), dict(points=odd),
           dict(out=odd), dict(calib=odd), dict(shape=odd), dict(status=odd), dict(box_off=odd), dict(box_cnt=odd),
           dict(boxes=ctypes.c_void_p(20)), dict(out_off=ctypes.c_void_p(20)), dict(scratch_bytes=8)]
    for kw in bad:
        assert _call(L, **kw) == EINVAL, kw
    for kw in (dict(n_rows=C['DFU3D_ING_MAX_ROWS'] + 1), dict(B=C['DFU3D_ING_MAX_SCENES'] + 1),
               dict(C=C['DFU3D_ING_MAX_POINT_COLS'] + 1), dict(n_boxes=C['DFU3D_ING_MAX_BOXES'] + 1)):
        assert _call(L, **kw) == ERANGE, kw
    # what a mode does not use is not looked at
    assert _call(L, mode=1, boxes=None, box_off=None, box_cnt=None, scratch_bytes=8) == EINVAL      # ... but the scratch is


def test_scratch_bytes():
    L = _lib_ingest.lib()
    C = _lib_ingest.CONSTANTS
    ch = C['DFU3D_ING_CHUNK']
    assert L.dfu3d_fov_ingest_scratch_bytes(-1) == 0 and L.dfu3d_fov_ingest_scratch_bytes(C['DFU3D_ING_MAX_ROWS'] + 1) == 0
    assert L.dfu3d_fov_ingest_scratch_bytes(0) == 8 + 16                    # one chunk even for no row
    for n in (1, ch, ch + 1, 34720 * 4):
        chunks = (n + ch - 1) // ch
        assert L.dfu3d_fov_ingest_scratch_bytes(n) == 8 * chunks + (n + 15) // 16 * 16 + 16


def _operands(n=10, C=4, B=2, m=3):
    import torch
    return dict(points=torch.zeros(n, C), point_off=torch.tensor([0] * B + [n]), calib=torch.zeros(B, 48),
                image_shape=torch.ones(B, 2, dtype=torch.int32), boxes=torch.zeros(m, 7, dtype=torch.float64),
                box_off=torch.tensor([0] * B + [m], dtype=torch.int32), mode=3)


def test_fov_ingest_validates_its_arguments():
    import torch
    from dfu3d_amd.ingest_ops import fov_ingest
    from dfu3d_amd._lib import Dfu3dError
    cases = [
        (dict(points=torch.zeros(10, 4, dtype=torch.float64)), "points must be float32"),
        (dict(points=np.zeros((10, 4), np.float32)), "points must be a tensor"),
        (dict(points=torch.zeros(10, 2)), "3 .. 64 columns, got 2"),
        (dict(points=torch.zeros(40)), r"points must be \(n, n\)"),
        (dict(points=torch.zeros(10, 8)[:, :4]), "points must be contiguous"),
        (dict(point_off=torch.tensor([0, 10])), r"point_off must be \(3\)"),
        (dict(point_off=torch.tensor([0, 5, 10], dtype=torch.int32)), "point_off must be int64"),
        (dict(calib=torch.zeros(2, 47)), r"calib must be \(n, 48\)"),
        (dict(image_shape=torch.ones(2, 2, dtype=torch.int64)), "image_shape must be int32"),
        (dict(image_shape=torch.ones(3, 2, dtype=torch.int32)), r"image_shape must be \(2, 2\)"),
        (dict(boxes=torch.zeros(3, 8, dtype=torch.float64)), r"boxes must be \(n, 7\)"),
        (dict(boxes=torch.zeros(3, 7)), "boxes must be float64"),
        (dict(boxes=torch.zeros(7, 3, dtype=torch.float64).t()), "boxes must be contiguous"),
        (dict(box_off=torch.tensor([0, 3], dtype=torch.int32)), r"box_off must be \(3\)"),
        (dict(box_off=torch.tensor([0, 1, 3])), "box_off must be int32"),
        (dict(boxes=None), "needs boxes and box_off"),
        (dict(mode=0), "mode must be"), (dict(mode=4), "mode must be"),
        (dict(status=torch.zeros(2, dtype=torch.int32)), r"status must be \(1\)"),
        (dict(), "points must be on the GPU"),                             # all well but the device: host tensors
    ]
    for change, text in cases:
        kw = dict(_operands(), **change)
        with pytest.raises(Dfu3dError, match=text):
            fov_ingest(**kw)
    # without DFU3D_ING_COUNT the boxes are not looked at
    with pytest.raises(Dfu3dError, match="on the GPU"):
        fov_ingest(**dict(_operands(), mode=1, boxes="no boxes", box_off=None))


# ---- the restatement against the reference (G18) ----
def test_ingest_ref_equals_the_reference(G):
    from dfu3d_amd.pcdet_kitti import box_utils
    from dfu3d_amd.pcdet_kitti.kitti_dataset import KittiDataset
    frames = K.golden_frames(G)
    assert len(frames) == 3
    kept_any = dropped_any = False
    for i, f in enumerate(frames):
        p = 'f%d_' % i
        calib = K.calib_of(f)
        flag = R.fov_flag(f['points'], calib, f['shape'])
        assert np.array_equal(flag, G[p + 'fov_flag']) and flag.dtype == np.bool_
        assert np.array_equal(flag, KittiDataset.get_fov_flag(calib.lidar_to_rect(f['points'][:, :3]), f['shape'], calib))
        kept_any, dropped_any = kept_any or flag.any(), dropped_any or not flag.all()
        boxes = G[p + 'ann_gt_boxes_lidar']
        n_obj = len(boxes)
        cnt = R.box_counts(f['points'][flag], boxes)
        assert np.array_equal(cnt, G[p + 'ann_num_points_in_gt'][:n_obj]) and cnt.dtype == np.int32
        assert (G[p + 'ann_num_points_in_gt'][n_obj:] == -1).all()
        if n_obj:
            assert cnt.min() > 0
            d = K.face_distance(f['points'], boxes)
            assert d[..., 0].min() >= K.BAND_XY and d[..., 1].min() >= K.BAND_Z
        got = box_utils.boxes3d_kitti_camera_to_lidar(G[p + 'boxes_camera'], calib)
        want = G[p + 'getitem_boxes']
        assert got.shape == want.shape and np.array_equal(got, want)
        assert got.dtype == want.dtype == np.float32 or len(want) == 0      # (the capture records no dtype for no box)
    assert kept_any and dropped_any
    out, off, flags, cnt = R.fov_ingest([f['points'] for f in frames], [K.calib_of(f) for f in frames],
                                        [f['shape'] for f in frames], [G['f%d_ann_gt_boxes_lidar' % i] for i in range(3)])
    assert off.tolist() == np.concatenate([[0], np.cumsum([int(G['f%d_fov_flag' % i].sum()) for i in range(3)])]).tolist()
    assert np.array_equal(out, np.concatenate([f['points'][G['f%d_fov_flag' % i]] for i, f in enumerate(frames)]))
    assert len(cnt) == sum(len(G['f%d_ann_gt_boxes_lidar' % i]) for i in range(3))


# ---- KittiDataset: the host logic ----
def _cfg(**over):
    cfg = {'DATA_SPLIT': {'train': 'train', 'test': 'val'}, 'INFO_PATH': {'train': ['kitti_infos_train.pkl'],
                                                                          'test': ['kitti_infos_val.pkl']},
           'FOV_POINTS_ONLY': True}
    cfg.update(over)
    return cfg


def _ref_counts(ds):
    def count(frames, batch_frames=16):
        out = []
        for sid, shape, boxes in frames:
            calib = ds.get_calib(sid)
            pts = ds.get_lidar(sid)
            out.append(R.box_counts(pts[R.fov_flag(pts, calib, shape)], boxes))
        return out
    return count


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def test_kitti_dataset_host_logic(tmp_path, G):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import KittiDataset
    frames = K.golden_frames(G)
    root = K.write_kitti(tmp_path, frames, split='train')
    ds = KittiDataset(_cfg(), K.CLASSES, training=True, root_path=root)
    assert ds.split == 'train' and ds.sample_id_list == ['000000', '000001', '000002'] and ds.mode == 'train'
    assert ds.kitti_infos == [] and len(ds) == 0                       # no info file yet
    # a split without an ImageSets file: no list, as in the reference
    assert KittiDataset(_cfg(), K.CLASSES, training=False, root_path=root).sample_id_list is None
    ds.set_split('nope')
    assert ds.split == 'nope' and ds.sample_id_list is None
    ds.set_split('train')
    assert ds.sample_id_list == ['000000', '000001', '000002']
    # the getters
    assert _same(ds.get_lidar('000002').view(np.uint32), frames[2]['points'].view(np.uint32))
    assert _same(ds.get_image_shape('000002'), np.array([900, 1600], np.int32))
    assert ds.get_label('000001') == [] and [o.cls_type for o in ds.get_label('000000')][-1] == 'DontCare'
    assert ds.get_road_plane('000000') is None
    with pytest.raises(FileNotFoundError):
        ds.get_lidar('000009')
    os.makedirs(os.path.join(root, 'planes'))
    with open(os.path.join(root, 'planes', '000000.txt'), 'w') as f:
        f.write("# Plane\nWidth 4\nHeight 1\n0.0 2.0 0.0 -3.0\n")
    assert ds.get_road_plane('000000').tolist() == [0.0, -1.0, 0.0, 1.5]
    # the infos against the reference's, the count through the NumPy restatement (the GPU form: tests/test_gpu_kitti_dataset.py)
    ds._count_inside = _ref_counts(ds)
    infos = ds.get_infos(num_workers=2)
    assert len(infos) == 3
    for i, info in enumerate(infos):
        p = 'f%d_' % i
        assert info['point_cloud'] == {'num_features': 4, 'lidar_idx': frames[i]['id']}
        assert info['image']['image_idx'] == frames[i]['id'] and _same(info['image']['image_shape'], G[p + 'image_shape'])
        for k in ('P2', 'R0_rect', 'Tr_velo_to_cam'):
            assert _same(info['calib'][k], G[p + 'calib_' + k]), k
        assert list(info['annos']) == list(K.INFO_KEYS)
        for k in K.INFO_KEYS:
            want = G[p + 'ann_' + k]
            if k == 'name':                                             # recorded as text; an empty one is float64 there
                assert info['annos'][k].tolist() == want.tolist() and (len(want) or info['annos'][k].dtype == np.float64)
            else:
                assert _same(info['annos'][k], want), (i, k, info['annos'][k], want)
    assert infos[0]['annos']['num_points_in_gt'][-1] == -1 and infos[0]['annos']['index'][-1] == -1     # the DontCare row
    assert infos[1]['annos']['name'].shape == (0,) and infos[1]['annos']['gt_boxes_lidar'].shape == (0, 7)  # the empty file
    without = ds.get_infos(count_inside_pts=False, sample_id_list=['000002'])
    assert len(without) == 1 and 'num_points_in_gt' not in without[0]['annos']
    assert 'annos' not in ds.get_infos(has_label=False, sample_id_list=['000001'])[0]
    # through pickle and back into a dataset
    with open(os.path.join(root, 'kitti_infos_train.pkl'), 'wb') as f:
        pickle.dump(infos, f)
    ds2 = KittiDataset(_cfg(), K.CLASSES, training=True, root_path=root)
    assert len(ds2) == 3 and all(_same(a['annos'][k], b['annos'][k]) for a, b in zip(ds2.kitti_infos, infos) for k in K.INFO_KEYS)
    # without the PNG the shape comes from the infos
    os.remove(os.path.join(root, 'image_2', '000002.png'))
    assert _same(ds2.get_image_shape('000002'), np.array([900, 1600], np.int32))
    with pytest.raises(FileNotFoundError):
        ds.get_image_shape('000002')
    # the host part of a frame: DontCare dropped, the reference's boxes
    for i in range(3):
        d, raw = ds2._frame(i)
        assert d['frame_id'] == frames[i]['id'] and _same(d['image_shape'], G['f%d_image_shape' % i])
        assert d['gt_names'].tolist() == G['f%d_getitem_names' % i].tolist() and 'DontCare' not in d['gt_names'].tolist()
        assert _same(d['gt_boxes'], G['f%d_getitem_boxes' % i]) or (len(d['gt_boxes']) == 0 and d['gt_boxes'].shape == (0, 7))
        assert _same(raw.view(np.uint32), frames[i]['points'].view(np.uint32))
    assert ('road_plane' in ds2._frame(0)[0]) and ('road_plane' not in ds2._frame(1)[0])
    # an entry this package does not have
    for entry in ('images', 'depth_maps', 'calib_matricies', 'gt_boxes2d'):
        bad = KittiDataset(_cfg(GET_ITEM_LIST=['points', entry]), K.CLASSES, training=True, root_path=root)
        with pytest.raises(NotImplementedError, match=entry):
            bad[0]
        with pytest.raises(NotImplementedError, match=entry):
            next(iter(bad.batches(2)))
    # an attribute object as the configuration
    from tests.centerpoint_cases import cfg as attr_cfg
    assert len(KittiDataset(attr_cfg(_cfg()), K.CLASSES, training=True, root_path=root)) == 3
    # evaluation without annotations
    ds3 = KittiDataset(_cfg(), K.CLASSES, training=False, root_path=root)
    assert ds3.evaluation([], K.CLASSES) == (None, {})
    b = ds2.batches(2)
    assert len(b) == 2 and b.dataset is ds2 and len(ds2.batches(2, drop_last=True)) == 1


def test_eval_one_epoch_refuses_dist_test(tmp_path):
    from dfu3d_amd.eval_utils.eval_utils import eval_one_epoch
    with pytest.raises(NotImplementedError, match="dist_test"):
        eval_one_epoch({}, {}, None, None, 0, None, dist_test=True, result_dir=tmp_path)
