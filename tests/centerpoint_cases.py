"""Configurations shared by tests/golden/capture_centerpoint_golden.py and the CenterPoint tests: the small model of
golden G16(b) and of tests/test_gpu_centerpoint.py, the full model of centerpoint_nuscenes2kitti.yaml (the values of the
config file, typed in here as plain dicts), and the scatter cases of G16(a)."""
import os

import numpy as np

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g16_centerpoint.npz")


class Cfg(dict):
    """A dict with attribute access, as the reference's EasyDict configs have."""
    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name)


def cfg(d):
    if isinstance(d, dict):
        return Cfg({k: cfg(v) for k, v in d.items()})
    if isinstance(d, (list, tuple)):
        return [cfg(v) for v in d]
    return d


HEAD_DICT = {'center': {'out_channels': 2, 'num_conv': 2}, 'center_z': {'out_channels': 1, 'num_conv': 2},
             'dim': {'out_channels': 3, 'num_conv': 2}, 'rot': {'out_channels': 2, 'num_conv': 2}}


def dense_head_cfg(heads, shared, stride, num_max_objs, k, post_max):
    return {'NAME': 'CenterHead', 'CLASS_AGNOSTIC': False, 'CLASS_NAMES_EACH_HEAD': heads, 'SHARED_CONV_CHANNEL': shared,
            'USE_BIAS_BEFORE_NORM': True, 'NUM_HM_CONV': 2,
            'SEPARATE_HEAD_CFG': {'HEAD_ORDER': ['center', 'center_z', 'dim', 'rot'], 'HEAD_DICT': HEAD_DICT},
            'TARGET_ASSIGNER_CONFIG': {'FEATURE_MAP_STRIDE': stride, 'NUM_MAX_OBJS': num_max_objs, 'GAUSSIAN_OVERLAP': 0.1,
                                       'MIN_RADIUS': 2},
            'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 0.25, 'code_weights': [1.0] * 8}},
            'POST_PROCESSING': {'SCORE_THRESH': 0.1, 'POST_CENTER_LIMIT_RANGE': [0, -61.2, -10.0, 61.2, 61.2, 10.0],
                                'MAX_OBJ_PER_SAMPLE': k,
                                'NMS_CONFIG': {'MULTI_CLASSES_NMS': True, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.6,
                                               'NMS_PRE_MAXSIZE': 1000, 'NMS_POST_MAXSIZE': post_max}}}


# ---- centerpoint_nuscenes2kitti.yaml ----
FULL_CLASSES = ['Car', 'Truck', 'Construction_vehicle', 'Bus', 'Trailer', 'Barrier', 'Motorcycle', 'Bicycle', 'Pedestrian',
                'Traffic_cone']
FULL_MODEL = {
    'NAME': 'CenterPoint',
    'VFE': {'NAME': 'DynPillarVFE', 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': [64, 64]},
    'MAP_TO_BEV': {'NAME': 'PointPillarScatter', 'NUM_BEV_FEATURES': 64},
    'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [3, 5, 5], 'LAYER_STRIDES': [2, 2, 2],
                    'NUM_FILTERS': [64, 128, 256], 'UPSAMPLE_STRIDES': [0.5, 1, 2], 'NUM_UPSAMPLE_FILTERS': [128, 128, 128]},
    'DENSE_HEAD': dense_head_cfg([['Car'], ['Truck', 'Construction_vehicle'], ['Bus', 'Trailer'], ['Barrier'],
                                  ['Motorcycle', 'Bicycle'], ['Pedestrian', 'Traffic_cone']], 64, 4, 500, 500, 83),
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'EVAL_METRIC': 'kitti'},
}
FULL_DATASET = dict(class_names=FULL_CLASSES, point_cloud_range=[0, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 8.0],
                    grid_size=[256, 512, 1], num_point_features=4)

# ---- the small model: G16(b) on the CPU, tests/test_gpu_centerpoint.py on the GPU ----
SMALL_CLASSES = ['Car', 'Pedestrian', 'Cyclist']
SMALL_MODEL = {
    'NAME': 'CenterPoint',
    'VFE': {'NAME': 'DynPillarVFE', 'WITH_DISTANCE': False, 'USE_ABSLOTE_XYZ': True, 'USE_NORM': True, 'NUM_FILTERS': [8, 8]},
    'MAP_TO_BEV': {'NAME': 'PointPillarScatter', 'NUM_BEV_FEATURES': 8},
    'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [1, 2, 2], 'LAYER_STRIDES': [2, 2, 2],
                    'NUM_FILTERS': [8, 16, 32], 'UPSAMPLE_STRIDES': [0.5, 1, 2], 'NUM_UPSAMPLE_FILTERS': [8, 8, 8]},
    'DENSE_HEAD': dense_head_cfg([['Car'], ['Pedestrian', 'Cyclist']], 8, 4, 20, 50, 20),
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'EVAL_METRIC': 'kitti'},
}
# 64 x 48 pillars of 0.5 m
SMALL_DATASET = dict(class_names=SMALL_CLASSES, point_cloud_range=[0.0, -12.0, -3.0, 32.0, 12.0, 1.0],
                     voxel_size=[0.5, 0.5, 4.0], grid_size=[64, 48, 1], num_point_features=4)
SMALL_INPUT = (2, 8, 24, 32)             # G16(b)'s spatial_features

# ---- G16(a): (name, class, B, C, (nx, ny, nz), P, seed) ----
SCATTER_CASES = [('s0', 'PointPillarScatter', 3, 64, (70, 37, 1), 300, 161),
                 ('s1', 'PointPillarScatter', 2, 5, (16, 9, 1), 144 * 2, 162),          # fully occupied
                 ('s2', 'PointPillarScatter3d', 2, 8, (23, 19, 4), 900, 163)]
GRAD_CASE = 's0'


def scatter_inputs(B, C, grid, P, seed, empty=(), corners=()):
    """P distinct cells in random order over the samples not in `empty`, the four (y, x) corners of the samples in
    `corners` among them; features with a NaN, an infinity and a -0.0 planted.  -> features (P, C), coords (P, 4) int32."""
    nx, ny, nz = grid
    rng = np.random.default_rng(seed)
    vol = nz * ny * nx
    live = [b for b in range(B) if b not in empty]
    must = [(b * nz + 0) * ny * nx + y * nx + x for b in corners for y in (0, ny - 1) for x in (0, nx - 1)]
    must = sorted(set(must))
    pool = np.setdiff1d(np.concatenate([np.arange(b * vol, (b + 1) * vol) for b in live]), must)
    pick = np.concatenate([np.array(must, np.int64), rng.choice(pool, size=P - len(must), replace=False)])
    pick = pick[rng.permutation(P)]
    coords = np.stack([pick // vol, pick % vol // (ny * nx), pick % (ny * nx) // nx, pick % nx], 1).astype(np.int32)
    f = rng.standard_normal((P, C)).astype(np.float32)
    if P * C >= 3:
        flat = f.reshape(-1)
        flat[0], flat[1], flat[2] = np.float32(np.nan), np.float32(np.inf), np.float32(-0.0)
    return f, coords


def golden():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}
