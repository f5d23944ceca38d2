"""Golden G26 (tests/golden/capture_pvrcnn_golden.py: the reference's VoxelSetAbstraction, PointHeadSimple and
PVRCNNHead on the CPU) against the NumPy restatements of tests/point_stack_ref.py -- every integer, and every bit of the
BEV-interpolated features -- and against the state-dict keys of this package's three modules.  No GPU."""
import os

import json

import numpy as np
import pytest

from tests import point_stack_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g26_pvrcnn.npz")
F32 = np.float32
SOURCES = ['raw_points', 'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4']


@pytest.fixture(scope="module")
def g26():
    return np.load(GOLDEN)


def meta_of(g):
    return json.loads(bytes(g['meta']).decode())


def voxel_centers(indices, factor):
    """(coords + 0.5) * (voxel_size * factor) + range, float32, in that order; indices (n, 4) [b, z, y, x]."""
    size = np.asarray(R.G26_VOXEL, F32) * F32(factor)
    return (indices[:, [3, 2, 1]].astype(F32) + F32(0.5)) * size + np.asarray(R.G26_RANGE[:3], F32)


def source_of(g, src):
    """-> xyz (n, 3), start (B + 1), features (n, C) of one feature source of the golden's fixture."""
    if src == 'raw_points':
        pts = g['points']
        return pts[:, 1:4], R.counts(pts[:, 0], R.G26_B)[1], pts[:, 4:]
    ind = g[src + '_indices']
    cnt, start, st = R.counts(ind[:, 0], R.G26_B)
    assert st == 0
    return voxel_centers(ind, R.G26_PFE['SA_LAYER'][src]['DOWNSAMPLE_FACTOR']), start, g[src + '_features']


def test_golden_is_small_and_has_the_fixture(g26):
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "g20_pointrcnn.npz"))
    cnt, start, st = R.counts(g26['points'][:, 0], R.G26_B)
    assert st == 0 and cnt.tolist() == R.G26_COUNTS and min(R.G26_COUNTS) < R.G26_PFE['NUM_KEYPOINTS']
    assert g26['spatial_features'].shape == (R.G26_B,) + R.G26_BEV and g26['rois'].shape == (R.G26_B, R.G26_ROIS, 7)
    assert g26['empty_roi_grid_0'].any() and not g26['empty_roi_grid_0'].all()


def test_restatement_equals_the_golden_integers_and_the_bilinear_bits(g26):
    K = R.G26_PFE['NUM_KEYPOINTS']
    xyz, start, _ = source_of(g26, 'raw_points')
    idx, kp, st = R.fps(xyz, start, K)
    assert st == 0 and np.array_equal(kp.view(np.uint32), g26['point_coords'].view(np.uint32))
    assert np.array_equal(idx[1, 40:], idx[1, :8])                            # the short sample cycles
    cstart = R.starts([K] * R.G26_B)
    for src in SOURCES:
        sxyz, sstart, _ = source_of(g26, src)
        cfg = R.G26_PFE['SA_LAYER'][src]
        for s, (r, ns) in enumerate(zip(cfg['POOL_RADIUS'], cfg['NSAMPLE'])):
            want_idx, want_empty = R.ball_query(sxyz, sstart, kp[:, 1:4], cstart, r, ns)
            assert np.array_equal(want_idx, g26['ball_%s_%d' % (src, s)]), (src, s)
            assert np.array_equal(want_empty, g26['empty_%s_%d' % (src, s)]), (src, s)
    bev = R.bev_sample(kp, g26['spatial_features'], R.G26_RANGE, R.G26_VOXEL, R.G26_BEV_STRIDE)
    assert np.array_equal(bev.view(np.uint32), g26['bev_features'].view(np.uint32))
    assert np.array_equal(bev.view(np.uint32), g26['point_features_before_fusion'][:, :R.G26_BEV[0]].view(np.uint32))
    # the RoI grid: the golden's global grid points as centres, the keypoints as the points
    pool = R.G26_ROI_HEAD['ROI_GRID_POOL']
    grid = g26['global_grid_points'].reshape(-1, 3)
    gstart = R.starts([len(grid) // R.G26_B] * R.G26_B)
    for s, (r, ns) in enumerate(zip(pool['POOL_RADIUS'], pool['NSAMPLE'])):
        want_idx, want_empty = R.ball_query(kp[:, 1:4], cstart, grid, gstart, r, ns)
        assert np.array_equal(want_idx, g26['ball_roi_grid_%d' % s]) and np.array_equal(want_empty, g26['empty_roi_grid_%d' % s])


def test_state_dict_keys_equal_the_golden(g26):
    from dfu3d_amd.pcdet_kitti.point_head_simple import PointHeadSimple
    from dfu3d_amd.pcdet_kitti.pvrcnn_head import PVRCNNHead
    from dfu3d_amd.pcdet_kitti.voxel_set_abstraction import VoxelSetAbstraction
    meta = meta_of(g26)
    pfe = VoxelSetAbstraction(R.G26_PFE, R.G26_VOXEL, R.G26_RANGE, num_bev_features=R.G26_BEV[0], num_rawpoint_features=4)
    head = PointHeadSimple(1, pfe.num_point_features_before_fusion, R.G26_POINT_HEAD)
    roi = PVRCNNHead(pfe.num_point_features, R.G26_ROI_HEAD, 1)
    assert R.G26_PFE['SA_LAYER']['x_conv2']['MLPS'] == [[8, 8], [8, 8]]        # the configuration is not written to
    for tag, model in (('pfe', pfe), ('point_head', head), ('roi_head', roi)):
        own = model.state_dict()
        gold = [k for k in meta[tag + '_keys'] if not k.startswith(('reg_loss_func', 'cls_loss_func'))]
        assert list(own) == gold, tag
        for k, v in own.items():
            assert tuple(v.shape) == g26['sd_%s_%s' % (tag, k)].shape, (tag, k)


def test_modules_refuse_what_is_not_part_of_the_package():
    from dfu3d_amd.pcdet_kitti import pointnet2_stack_modules as M
    from dfu3d_amd.pcdet_kitti.voxel_set_abstraction import VoxelSetAbstraction
    with pytest.raises(NotImplementedError, match="VectorPoolAggregationModuleMSG"):
        M.build_local_aggregation_module(4, {'NAME': 'VectorPoolAggregationModuleMSG'})
    with pytest.raises(NotImplementedError, match="SAMPLE_METHOD"):
        VoxelSetAbstraction(dict(R.G26_PFE, SAMPLE_METHOD='SPC'), R.G26_VOXEL, R.G26_RANGE, 8, 4)
    layers = dict(R.G26_PFE['SA_LAYER'], raw_points=dict(R.G26_PFE['SA_LAYER']['raw_points'], FILTER_NEIGHBOR_WITH_ROI=True))
    with pytest.raises(NotImplementedError, match="FILTER_NEIGHBOR_WITH_ROI"):
        VoxelSetAbstraction(dict(R.G26_PFE, SA_LAYER=layers), R.G26_VOXEL, R.G26_RANGE, 8, 4)
    from dfu3d_amd.pcdet_kitti.pv_rcnn import PVRCNN
    assert set(PVRCNN.MORE_MODULES) == {'DENSE_HEAD', 'PFE', 'POINT_HEAD', 'ROI_HEAD'}
