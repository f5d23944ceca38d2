"""Sequential NumPy float32 restatement of both forms of the RoI-point pooling of include/dfu3d_roi.h, and the case table
of its tests.  Importable without the reference and without a GPU.  Every array operation below is one float32 (or, where
the header says so, float64) operation per element, in the order of the header's expressions; the trig is evaluated in
float64 and rounded once."""
import collections

import numpy as np

F32, F64 = np.float32, np.float64
MARGIN = F32(1e-5)
TRIP, WAVE = 1024, 64                     # points of one trip of the search (sixteen tiles), of one of its tiles


def load_box(box, extra):
    """box float32 (7), extra (3) -> the constants of the in-box test."""
    box = np.asarray(box, F32)
    ex = np.asarray(extra, F32)
    with np.errstate(all='ignore'):
        dx, dy, dz = box[3] + ex[0], box[4] + ex[1], box[5] + ex[2]
        ang = -F64(box[6])
        return dict(cx=box[0], cy=box[1], cz=box[2], cosa=F32(np.cos(ang)), sina=F32(np.sin(ang)),
                    hz=F64(dz) / 2.0, hx=F64(dx) / 2.0 + F64(MARGIN), hy=F64(dy) / 2.0 + F64(MARGIN))


def local_xy(q, pts):
    """pts float32 (n, 3) -> lx, ly float32 (n): the rotation of the in-box test and of the canonical transform."""
    with np.errstate(all='ignore'):
        sx, sy = pts[:, 0] - q['cx'], pts[:, 1] - q['cy']
        return sx * q['cosa'] + sy * (-q['sina']), sx * q['sina'] + sy * q['cosa']


def in_box(q, pts):
    pts = np.asarray(pts, F32)
    with np.errstate(all='ignore'):
        z_out = np.abs(pts[:, 2] - q['cz']).astype(F64) > q['hz']
        lx, ly = local_xy(q, pts)
        return ~z_out & (np.abs(lx).astype(F64) < q['hx']) & (np.abs(ly).astype(F64) < q['hy'])


def search(points, boxes, extra, S):
    """-> pooled_idx int32 (B, M, S), pooled_empty_flag int32 (B, M), hits: per (b, m) ALL point indices inside."""
    points, boxes = np.asarray(points, F32), np.asarray(boxes, F32)
    B, M = boxes.shape[:2]
    idx, flag, hits = np.zeros((B, M, S), np.int32), np.zeros((B, M), np.int32), {}
    for b in range(B):
        for m in range(M):
            h = np.nonzero(in_box(load_box(boxes[b, m], extra), points[b]))[0]
            hits[b, m] = h
            cnt = min(len(h), S)
            if cnt == 0:
                flag[b, m] = 1
            else:
                idx[b, m] = h[np.arange(S) % cnt]
    return idx, flag, hits


def pool(points, features, boxes, extra, S):
    """The plain form -> pooled float32 (B, M, S, 3 + C), flag, idx."""
    points, features = np.asarray(points, F32), np.asarray(features, F32)
    idx, flag, _ = search(points, boxes, extra, S)
    B, M = flag.shape
    out = np.zeros((B, M, S, 3 + features.shape[2]), F32)
    for b in range(B):
        for m in range(M):
            if not flag[b, m]:
                ii = idx[b, m].astype(np.int64)
                out[b, m, :, :3] = points[b, ii]
                out[b, m, :, 3:] = features[b, ii]
    return out, flag, idx


def depth_of(points, normalizer):
    x, y, z = points[..., 0], points[..., 1], points[..., 2]
    with np.errstate(all='ignore'):
        return np.sqrt((x * x + y * y) + z * z) / F32(normalizer) - F32(0.5)


def pool_fused(points, scores, features, boxes, extra, S, normalizer):
    """The fused form -> pooled float32 (B * M, S, 5 + C), flag, idx."""
    points, features, scores = np.asarray(points, F32), np.asarray(features, F32), np.asarray(scores, F32)
    boxes = np.asarray(boxes, F32)
    idx, flag, _ = search(points, boxes, extra, S)
    B, M = flag.shape
    out = np.zeros((B, M, S, 5 + features.shape[2]), F32)
    for b in range(B):
        depth = depth_of(points[b], normalizer)
        for m in range(M):
            if flag[b, m]:
                continue
            ii = idx[b, m].astype(np.int64)
            q = load_box(boxes[b, m], (0.0, 0.0, 0.0))
            out[b, m, :, 0], out[b, m, :, 1] = local_xy(q, points[b, ii])
            with np.errstate(all='ignore'):
                out[b, m, :, 2] = points[b, ii, 2] - q['cz']
            out[b, m, :, 3], out[b, m, :, 4], out[b, m, :, 5:] = scores[b, ii], depth[ii], features[b, ii]
    return out.reshape(B * M, S, -1), flag, idx


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- the case table ---------------------------------------------------------------------------------------------------
Case = collections.namedtuple('Case', 'name points scores features boxes extra S normalizer')

# (B, N, M, S, C): every N, S, C and M of the list below occurs; B = 3 gives different clouds and boxes per sample
# N: below a wave, at and around 256 points, at and around a trip of the search, several trips
N_VALUES, S_VALUES, C_VALUES, M_VALUES = (1, 37, 64, 255, 256, 257, 600, 1023, 1024, 1025, 2600), (1, 5, 16, 64, 512), (0, 1, 13, 16, 128), (1, 5, 70)
RANDOM_SHAPES = [(3, 600, 70, 16, 13), (3, 257, 5, 5, 1), (3, 1, 1, 1, 0), (3, 37, 5, 64, 16), (3, 64, 1, 5, 128),
                 (3, 255, 5, 512, 0), (3, 256, 70, 64, 1), (3, 600, 5, 512, 128), (3, 1023, 5, 16, 1), (3, 1024, 5, 64, 0),
                 (3, 1025, 5, 5, 13)]


def _fill(rng, B, N, C):
    feats = rng.normal(0.0, 1.0, (B, N, C)).astype(F32)
    scores = rng.uniform(0.0, 1.0, (B, N)).astype(F32)
    return scores, feats


def random_case(seed, B, N, M, S, C):
    """Clouds within +-8 m, boxes of 1 .. 9 m among them with headings over all four quadrants; the extra width is
    non-zero for odd seeds."""
    rng = np.random.default_rng(seed)
    pts = rng.uniform(-8.0, 8.0, (B, N, 3)).astype(F32)
    pts[..., 2] *= F32(0.25)
    boxes = np.zeros((B, M, 7), F32)
    boxes[..., :2] = rng.uniform(-6.0, 6.0, (B, M, 2))
    boxes[..., 2] = rng.uniform(-1.0, 1.0, (B, M))
    boxes[..., 3:6] = rng.uniform(1.0, 9.0, (B, M, 3))
    boxes[..., 6] = rng.uniform(-np.pi, np.pi, (B, M))
    extra = (0.3, 0.2, 0.1) if seed % 2 else (0.0, 0.0, 0.0)
    scores, feats = _fill(rng, B, N, C)
    return Case('random B%d N%d M%d S%d C%d' % (B, N, M, S, C), pts, scores, feats, boxes, extra, S, 70.0)


def counts_case():
    """S = 8, N = 2600 (two trips of the search and a partial one), three samples with their own clouds; sample 0 holds
    one RoI per count situation: the chosen point indices sit well inside their RoI's box, everything else is far from
    every box."""
    rng = np.random.default_rng(2015)
    B, N, S, C = 3, 2600, 8, 5
    pts = np.zeros((B, N, 3), F32)
    pts[..., 0] = rng.uniform(30.0, 60.0, (B, N))
    pts[..., 1:] = rng.uniform(-3.0, 3.0, (B, N, 2))
    members = [[],                                            # cnt = 0
               [417],                                         # cnt = 1: every slot the same point
               [5, 130, 599],                                 # cnt = 3 of S = 8: the k % cnt wrap
               [0, 63, 65, 254, 257, 319, 1023, 1030],        # cnt = S exactly
               [3, 9, 70, 71, 100, 101, 110, 157, 158, 300, 590],   # cnt > S, the S-th hit (157) in the middle of a wave
               [1, 2, 60, 64, 128, 191, 255, 256, 258, 400],  # cnt > S, the S-th hit the first point after 256
               [11, 200, 500, 700, 900, 1000, 1022, 1024, 1500, 2599],    # cnt > S, the S-th hit the first point of the next trip
               [2048, 2049, 2300, 2598]]                      # hits only in the last, partial trip
    M = len(members)
    assert len({i for t in members for i in t}) == sum(len(t) for t in members)
    boxes = np.zeros((B, M, 7), F32)
    for b in range(B):
        for m in range(M):
            boxes[b, m] = [-10.0 * (m + 1), 4.0 * b, 0.5 * m, 2.0, 2.0, 2.0, 0.7 * m - 2.0 + b]
            take = members[(m + b) % M]                       # the other samples: the same situations at other RoIs
            pts[b, take] = boxes[b, m, :3] + rng.uniform(-0.45, 0.45, (len(take), 3)).astype(F32)
    scores, feats = _fill(rng, B, N, C)
    return Case('counts', pts, scores, feats, boxes, (0.0, 0.0, 0.0), S, 70.0)


def faces_case():
    """Decisions that do not depend on trig: heading 0, dyadic coordinates, box centres with x = y = 0 so that lx = x and
    ly = y exactly.  Also the all-zero padded RoI with (sample 0) and without (sample 1) a point at the origin, a NaN
    point, a NaN box and an infinite dim."""
    B, N, S, C = 3, 37, 16, 1
    rng = np.random.default_rng(77)
    pts = np.zeros((B, N, 3), F32)
    pts[..., 0] = rng.uniform(40.0, 50.0, (B, N))             # far from every box below
    pts[..., 1:] = rng.uniform(-1.0, 1.0, (B, N, 2))
    hx = F64(F32(2.0)) / 2.0 + F64(MARGIN)                    # dx = 2: the x face of the in-box test
    below = F32(hx) if F64(F32(hx)) < hx else np.nextafter(F32(hx), F32(0.0))
    above = np.nextafter(below, F32(2.0))
    assert F64(below) < hx <= F64(above)
    boxes = np.zeros((B, 5, 7), F32)
    for b in range(B):
        boxes[b, 0] = [0.0, 0.0, 0.25, 2.0, 1.0, 0.5, 0.0]    # faces at z = 0 and 0.5, |x| < 1 + 1e-5, |y| < 0.5 + 1e-5
        boxes[b, 2] = [0.0, 0.0, 8.0, np.inf, 1.0, 1.0, 0.0]  # an infinite dim: every x
        boxes[b, 3] = [np.nan, 0.0, 0.0, 2.0, 2.0, 2.0, 0.0]  # a NaN box: empty
        boxes[b, 4] = [0.0, 0.0, -8.0, 2.0, 2.0, 2.0, 0.0] if b else [0.0, 0.0, -8.0, 2.0, 2.0, 2.0, np.nan]
        pts[b, 3] = [0.5, 0.25, 0.5]                          # exactly on z = cz + dz / 2: inside
        pts[b, 7] = [-0.5, -0.25, 0.0]                        # exactly on z = cz - dz / 2: inside
        pts[b, 11] = [1.0, 0.0, 0.25]                         # |lx| = dx / 2: inside (the margin)
        pts[b, 12] = [-below, 0.5, 0.25]                      # the last float inside in x, |ly| = dy / 2
        pts[b, 13] = [above, 0.0, 0.25]                       # one float step beyond dx / 2 + 1e-5: outside
        pts[b, 14] = [0.0, 0.0, np.nextafter(F32(0.5), F32(1.0))]      # one float step above the z face: outside
        pts[b, 20] = [123.0, 0.25, 8.25]                      # inside the infinite box only
        pts[b, 21] = [np.nan, 0.0, 8.0]                       # a NaN point: in no box, not even the infinite one
        pts[b, 22] = [0.25, 0.25, -8.0]                       # inside box 4 unless its heading is NaN
    pts[0, 30] = [0.0, 0.0, 0.0]                              # the origin: inside the all-zero RoI (box 1) of sample 0 ...
    pts[0, 31] = [0.0, 0.0, 0.0]
    pts[2, 30] = [0.0, 0.0, 0.0]                              # ... and of sample 2; sample 1 has no such point
    scores, feats = _fill(rng, B, N, C)
    return Case('faces', pts, scores, feats, boxes, (0.0, 0.0, 0.0), S, 70.0)


def extra_case():
    """A non-zero pool_extra_width decides: points 0.1 outside the bare box in each axis."""
    B, N, S, C = 3, 64, 5, 16
    rng = np.random.default_rng(99)
    pts = np.zeros((B, N, 3), F32)
    pts[..., 0] = rng.uniform(40.0, 50.0, (B, N))
    boxes = np.zeros((B, 1, 7), F32)
    for b in range(B):
        boxes[b, 0] = [1.0 + b, -2.0, 0.5, 2.0, 1.0, 1.0, 0.0]
        c = boxes[b, 0, :3]
        pts[b, 5] = c + np.array([1.1, 0.0, 0.0], F32)        # dx / 2 = 1: inside with 0.4 added to dx
        pts[b, 9] = c + np.array([0.0, -0.6, 0.0], F32)       # dy / 2 = 0.5
        pts[b, 40] = c + np.array([0.0, 0.0, 0.6], F32)       # dz / 2 = 0.5
        pts[b, 41] = c + np.array([1.3, 0.0, 0.0], F32)       # outside even so
    scores, feats = _fill(rng, B, N, C)
    return Case('extra', pts, scores, feats, boxes, (0.4, 0.4, 0.4), S, 35.0)


def cases():
    out = [random_case(300 + i, *shape) for i, shape in enumerate(RANDOM_SHAPES)]
    return out + [counts_case(), faces_case(), extra_case()]


def situations(case):
    """What the restatement alone finds in a case: a Counter over the situations the tests must meet."""
    n = collections.Counter()
    pts, boxes, S = case.points, case.boxes, case.S
    B, N = pts.shape[:2]
    _, flag, hits = search(pts, boxes, case.extra, S)
    bare = search(pts, boxes, (0.0, 0.0, 0.0), S)[2] if any(case.extra) else hits
    last_trip = (N - 1) // TRIP * TRIP
    for (b, m), h in hits.items():
        T, box = len(h), boxes[b, m]
        n['cnt0'] += T == 0
        n['cnt1'] += T == 1 and S > 1
        n['wrap'] += 1 < T < S and S % T != 0
        n['exact'] += T == S and S > 1
        if T > S:
            n['mid_wave'] += 0 < h[S - 1] % WAVE < WAVE - 1
            n['next_trip'] += h[S - 1] > 0 and h[S - 1] % TRIP == 0
            n['after_256'] += h[S - 1] == 256
        n['last_trip_only'] += T > 0 and N > TRIP and N % TRIP != 0 and h[0] >= last_trip
        n['extra_decides'] += len(h) > len(bare[b, m])
        zero = not box.any()
        n['zero_roi_hit'] += zero and T > 0
        n['zero_roi_empty'] += zero and T == 0
        n['nan_box'] += bool(np.isnan(box).any()) and T == 0
        n['inf_dim'] += bool(np.isinf(box[3:6]).any()) and T > 0
        if np.isfinite(box).all() and box[3:6].all():
            n['quadrant%d' % (int(np.floor(F64(box[6]) / (np.pi / 2))) % 4)] += 1
        if box[6] == 0 and np.isfinite(box).all():
            q = load_box(box, case.extra)
            with np.errstate(all='ignore'):
                lx, _ = local_xy(q, pts[b])
                dz = np.abs(pts[b, :, 2] - q['cz']).astype(F64)
                ax = np.abs(lx).astype(F64)
            inside = np.zeros(N, bool)
            inside[h] = True
            n['on_z_face_inside'] += int((inside & (dz == q['hz']) & (q['hz'] > 0)).sum())
            half = F64(box[3] + F32(case.extra[0])) / 2.0
            n['on_x_half_inside'] += int((inside & (ax == half) & (half > 0)).sum())
            n['last_float_inside'] += int((inside & (np.nextafter(np.abs(lx), F32(np.inf)).astype(F64) >= q['hx'])).sum())
            n['first_float_outside'] += int((~inside & (dz <= q['hz']) & (ax >= q['hx'])
                                             & (np.nextafter(np.abs(lx), F32(0.0)).astype(F64) < q['hx'])).sum())
    n['nan_point'] += int(np.isnan(pts).any(axis=-1).sum())
    n['batch_differs'] += B > 1 and not np.array_equal(pts[0], pts[-1]) and not np.array_equal(boxes[0], boxes[-1])
    return n


SITUATIONS = ('cnt0', 'cnt1', 'wrap', 'exact', 'mid_wave', 'next_trip', 'after_256', 'last_trip_only', 'extra_decides', 'zero_roi_hit',
              'zero_roi_empty', 'nan_box', 'inf_dim', 'quadrant0', 'quadrant1', 'quadrant2', 'quadrant3',
              'on_z_face_inside', 'on_x_half_inside', 'last_float_inside', 'first_float_outside', 'nan_point',
              'batch_differs')

# ---- the small model of golden G20 and the full configuration's model section ----------------------------------------
G20_CLASSES = ['Car', 'Pedestrian', 'Cyclist']
G20_B, G20_N = 2, 256
G20_EXTRA = 1                              # feature columns of the points beside x, y, z (the backbone of golden G19)
G20_MARGINS = {'score': 1e-4, 'iou': 1e-3, 'face': 1e-4}


def _heads(fc, xyz_up, sa, post, mean_size, pool):
    """The POINT_HEAD, ROI_HEAD and POST_PROCESSING sections of pointrcnn_nuscenes2kitti.yaml with the sizes given."""
    nms = lambda post_max, thresh: {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 9000,   # noqa: E731
                                    'NMS_POST_MAXSIZE': post_max, 'NMS_THRESH': thresh}
    return {
        'POINT_HEAD': {
            'NAME': 'PointHeadBox', 'CLS_FC': list(fc), 'REG_FC': list(fc), 'CLASS_AGNOSTIC': False,
            'USE_POINT_FEATURES_BEFORE_FUSION': False,
            'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2], 'BOX_CODER': 'PointResidualCoder',
                              'BOX_CODER_CONFIG': {'use_mean_size': True, 'mean_size': mean_size}},
            'LOSS_CONFIG': {'LOSS_REG': 'WeightedSmoothL1Loss',
                            'LOSS_WEIGHTS': {'point_cls_weight': 1.0, 'point_box_weight': 1.0, 'code_weights': [1.0] * 8}}},
        'ROI_HEAD': {
            'NAME': 'PointRCNNHead', 'CLASS_AGNOSTIC': True, 'ROI_POINT_POOL': pool, 'XYZ_UP_LAYER': list(xyz_up),
            'CLS_FC': list(fc), 'REG_FC': list(fc), 'DP_RATIO': 0.0, 'USE_BN': False, 'SA_CONFIG': sa,
            'NMS_CONFIG': {'TRAIN': nms(post[0], 0.8), 'TEST': nms(post[1], 0.85)},
            'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 128, 'FG_RATIO': 0.5,
                              'SAMPLE_ROI_BY_EACH_CLASS': True, 'CLS_SCORE_TYPE': 'cls', 'CLS_FG_THRESH': 0.6,
                              'CLS_BG_THRESH': 0.45, 'CLS_BG_THRESH_LO': 0.1, 'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
            'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                            'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                             'code_weights': [1.0] * 7}}},
        'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.1, 'OUTPUT_RAW_SCORE': False,
                            'EVAL_METRIC': 'kitti',
                            'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.1,
                                           'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
    }


def g20_model_cfg():
    """The small model: golden G19's backbone (16 point features out), heads of 16 channels, 16 pooled points, 12 RoIs."""
    from tests import pointnet2_ref
    return dict(NAME='PointRCNN', BACKBONE_3D=dict(NAME='PointNet2MSG', **pointnet2_ref.G19_CFG),
                **_heads(fc=[16], xyz_up=[16, 16], post=(12, 12),
                         sa={'NPOINTS': [8, -1], 'RADIUS': [1.0, 100.0], 'NSAMPLE': [4, 4], 'MLPS': [[16, 16], [16, 32]]},
                         mean_size=[[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]],
                         pool={'POOL_EXTRA_WIDTH': [0.2, 0.1, 0.1], 'NUM_SAMPLED_POINTS': 16, 'DEPTH_NORMALIZER': 70.0}))


FULL_CLASSES = ['Car', 'Truck', 'Construction_vehicle', 'Bus', 'Trailer', 'Motorcycle', 'Bicycle', 'Pedestrian']


def full_model_cfg():
    """The MODEL section of pointrcnn_nuscenes2kitti.yaml."""
    from tests import pointnet2_ref
    return dict(NAME='PointRCNN', BACKBONE_3D=dict(NAME='PointNet2MSG', **pointnet2_ref.FULL_CFG),
                **_heads(fc=[256, 256], xyz_up=[128, 128], post=(512, 100),
                         sa={'NPOINTS': [128, 32, -1], 'RADIUS': [0.2, 0.4, 100], 'NSAMPLE': [16, 16, 16],
                             'MLPS': [[128, 128, 128], [128, 128, 256], [256, 256, 512]]},
                         mean_size=[[4.63, 1.97, 1.74], [6.93, 2.51, 2.84], [6.37, 2.85, 3.19], [10.5, 2.94, 3.47],
                                    [12.29, 2.90, 3.87], [2.11, 0.77, 1.47], [1.70, 0.60, 1.28], [0.73, 0.67, 1.77]],
                         pool={'POOL_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'NUM_SAMPLED_POINTS': 512, 'DEPTH_NORMALIZER': 70.0}))
