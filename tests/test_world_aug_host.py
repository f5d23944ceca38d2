"""CPU: the host side of the world-augmentation row -- construction errors, DISABLE_AUG_LIST, the placeholder's grid size,
argument validation before any launch, and the agreement of include/dfu3d_aug.h with its binding."""
import ctypes
import os
import re

import numpy as np
import pytest

from dfu3d_amd import _build, _lib_aug
from dfu3d_amd._lib import Dfu3dError
from dfu3d_amd.pcdet_kitti.data_augmentor import DataAugmentor, class_ids, params_record, select_classes
from dfu3d_amd.pcdet_kitti.data_processor import DataProcessor

FLIP = {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x']}
ROT = {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [-0.5, 0.5]}
SCALE = {'NAME': 'random_world_scaling', 'WORLD_SCALE_RANGE': [0.95, 1.05]}
TRANS = {'NAME': 'random_world_translation', 'NOISE_TRANSLATE_STD': [0.5, 0.5, 0.5]}
RANGE = np.array([0, -39.68, -3, 69.12, 39.68, 1], np.float32)


def test_header_and_binding_agree():
    assert _lib_aug.HEADER == os.path.join(_build.INCLUDE, "dfu3d_aug.h") and _lib_aug.HEADER in _build._deps()
    assert _lib_aug.header_version() == 1
    assert _lib_aug.header_symbols() == ['dfu3d_aug_version', 'dfu3d_world_aug_collate', 'dfu3d_world_aug_scratch_bytes']
    text = open(_lib_aug.HEADER).read()
    proto = re.search(r"int dfu3d_world_aug_collate\((.*?)\);", text, re.S).group(1)
    res, args = _lib_aug.SIGNATURES['dfu3d_world_aug_collate']
    assert res is ctypes.c_int32 and len(args) == len(proto.split(","))
    P = _lib_aug.Params
    assert ctypes.sizeof(P) == 48 and P.noise_rot.offset == 32 and P.scale.offset == 40 and P.tx.offset == 20
    flags = [_lib_aug.CONSTANTS['DFU3D_AUG_' + n] for n in ('FLIP_X', 'FLIP_Y', 'ROTATE', 'SCALE', 'TRANSLATE', 'WRAP',
                                                            'FLIP_Y_FIRST')]
    assert flags == [1, 2, 4, 8, 16, 32, 64] and _lib_aug.CONSTANTS['DFU3D_AUG_CHUNK'] == 1024
    # the other headers do not know this one, and this one only adds to the library
    for other in ("dfu3d.h", "dfu3d_vfe.h", "dfu3d_head.h", "dfu3d_post.h"):
        assert "dfu3d_aug" not in open(os.path.join(_build.INCLUDE, other)).read()


def test_construction_errors_and_disable_list():
    with pytest.raises(NotImplementedError):
        DataAugmentor('.', [{'NAME': 'random_local_rotation', 'LOCAL_ROT_ANGLE': 0.1}], ['Car'])
    with pytest.raises(NotImplementedError):
        DataAugmentor('.', [ROT, FLIP], ['Car'])                       # the stage's order is fixed
    with pytest.raises(NotImplementedError):
        DataAugmentor('.', [dict(FLIP, ALONG_AXIS_LIST=['x', 'x'])], ['Car'])
    with pytest.raises(Dfu3dError):
        DataAugmentor('.', [dict(TRANS, NOISE_TRANSLATE_STD=[0.5])], ['Car'])
    a = DataAugmentor('.', {'AUG_CONFIG_LIST': [{'NAME': 'random_local_rotation'}, FLIP, ROT, SCALE, TRANS],
                            'DISABLE_AUG_LIST': ['random_local_rotation', 'random_world_scaling']}, ['Car'])
    assert a.data_augmentor_queue == ['random_world_flip', 'random_world_rotation', 'random_world_translation']
    assert a.sampler is None
    np.random.seed(3)
    d = a.draw_world_params(7)
    assert d['noise_scale'] is None and d['noise_translate'].shape == (1, 3) and len(d['flips']) == 1
    with pytest.raises(Dfu3dError):
        a.draw_world_params(8)
    with pytest.raises(NotImplementedError):
        DataProcessor([{'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': [0.1, 0.1, 0.1]}], RANGE, True, 4)
    with pytest.raises(NotImplementedError):
        DataProcessor([{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True,
                        'USE_CENTER_TO_FILTER': False}], RANGE, True, 4)
    with pytest.raises(NotImplementedError):
        DataProcessor([{'NAME': 'sample_points'}], RANGE, True, 4)


def test_narrow_scale_range_draws_nothing():
    a = DataAugmentor('.', [dict(SCALE, WORLD_SCALE_RANGE=[1.0, 1.0005]), TRANS], ['Car'])
    b = DataAugmentor('.', [TRANS], ['Car'])
    np.random.seed(9)
    x = a.draw_world_params()
    np.random.seed(9)
    y = b.draw_world_params()
    assert x['noise_scale'] is None and np.array_equal(x['noise_translate'], y['noise_translate'])


def test_params_record_and_class_ids():
    from dfu3d_amd import stages as st
    rec = params_record({'flips': [('y', True), ('x', False)], 'noise_rot': 0.25, 'noise_scale': None,
                         'noise_translate': np.array([[1, 2, 3]], np.float32)})
    assert rec['flags'] == st.AUG_WRAP | st.AUG_FLIP_Y | st.AUG_FLIP_Y_FIRST | st.AUG_ROTATE | st.AUG_TRANSLATE
    assert rec['noise_rot'] == 0.25 and (rec['tx'], rec['ty'], rec['tz']) == (1.0, 2.0, 3.0)
    assert np.float32(rec['cos_a']) == np.float32(np.cos(np.float32(0.25)))
    raw = st.aug_params([rec, {'flags': 0}])
    assert raw.shape == (2, 48) and raw.dtype == np.uint8
    assert np.frombuffer(raw[0, 32:40].tobytes(), np.float64)[0] == 0.25
    assert np.frombuffer(raw[1, 12:16].tobytes(), np.float32)[0] == 1.0          # the neutral scale
    with pytest.raises(Dfu3dError):
        st.aug_params([{'angle': 1.0}])
    assert list(class_ids(['Car', 'Van', 'Cyclist'], ['Car', 'Pedestrian', 'Cyclist'])) == [1, 0, 3]
    d = select_classes({'gt_boxes': np.zeros((3, 7)), 'gt_names': np.array(['Car', 'Van', 'Cyclist'])},
                       ['Car', 'Pedestrian', 'Cyclist'])
    assert d['gt_boxes'].shape == (2, 8) and d['gt_boxes'].dtype == np.float64 and list(d['gt_boxes'][:, 7]) == [1, 3]


def test_placeholder_grid_size_and_mask_mode():
    from dfu3d_amd import stages as st
    cfgs = [{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True},
            {'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': {'train': True, 'test': False}},
            {'NAME': 'transform_points_to_voxels_placeholder', 'VOXEL_SIZE': [0.32, 0.32, 4.0]}]
    p = DataProcessor(cfgs, RANGE, True, 4)
    assert list(p.grid_size) == [216, 248, 1] and p.grid_size.dtype == np.int64 and p.voxel_size == [0.32, 0.32, 4.0]
    assert p.mask_mode() == st.AUG_MASK_POINTS | st.AUG_MASK_BOXES
    assert DataProcessor(cfgs, RANGE, False, 4).mask_mode() == st.AUG_MASK_POINTS
    assert DataProcessor(cfgs[1:], RANGE, True, 4).mask_mode() == 0
    np.random.seed(4)
    want = np.random.permutation(5)
    np.random.seed(4)
    d = p.shuffle_points(data_dict={'points': np.arange(5, dtype=np.float32).reshape(5, 1)}, config=cfgs[1])
    assert list(d['points'][:, 0]) == list(want)


def test_arguments_are_validated_before_any_launch():
    """Everything below fails on the host, in the wrapper, before the library is even loaded (no GPU here)."""
    import torch
    from dfu3d_amd import stages as st
    z = torch.zeros
    ok = dict(points=z((4, 4)), point_off=z(2, dtype=torch.int64), boxes=z((2, 7)), box_off=z(2, dtype=torch.int32),
              box_cnt=z(1, dtype=torch.int32), box_cls=z(2, dtype=torch.int32), params=z((1, 48), dtype=torch.uint8),
              pc_range=z(6), mode=0, box_cap=2, status=z(1, dtype=torch.int32))
    for bad in (dict(points=z((4, 2))), dict(boxes=z((2, 8))), dict(boxes=z((2, 7), dtype=torch.float16)),
                dict(mode=8), dict(box_cap=-1), dict(box_cap=st.AUG_MAX_BOX_CAP + 1), dict(points=z((4, 65))),
                dict(points=np.zeros((4, 4), np.float32)), dict()):       # the last: host tensors are refused too
        with pytest.raises(Dfu3dError):
            st.world_aug_collate(**dict(ok, **bad))
    a = DataAugmentor('.', [FLIP], ['Car'])
    for pts, boxes in ((np.zeros((3, 4)), np.zeros((1, 7), np.float32)), (np.zeros((3, 4), np.float32), np.zeros((1, 8))),
                       (np.zeros((3, 2), np.float32), np.zeros((1, 7))), (np.zeros((3, 4), np.float32), np.zeros((1, 7), np.int64))):
        with pytest.raises(Dfu3dError):
            a.forward({'points': pts, 'gt_boxes': boxes, 'gt_names': np.array(['Car'])})
