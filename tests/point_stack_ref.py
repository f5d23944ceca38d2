"""Sequential NumPy float32 restatements of the five contracts of csrc/dfu3d_stk.h (stacked set abstraction), and the
case tables of their tests.  Importable without the reference, without the package and without a GPU.  Every array
operation below is one float32 operation per element, in the order of the C header's expressions."""
import numpy as np

F32 = np.float32

ST_BAD_POINT, ST_BAD_INDEX, ST_BAD_BATCH, ST_UNSORTED, ST_EMPTY, ST_BAD_COUNT = 1, 2, 4, 8, 16, 32

FPS_COUNTS, FPS_K = [700, 40, 1, 300], 64
FPS_BIG_COUNTS = [16500, 90]
BALL_N = [0, 1, 63, 64, 65, 700]
BALL_M = [5, 0, 3, 9, 2, 70]
BALL_NSAMPLE = [1, 16, 32]
GROUP_C = [0, 1, 16]

# the small model of golden G26
G26_B, G26_COUNTS = 2, [300, 40]
G26_RANGE = [0.0, -3.0, -1.0, 8.0, 3.0, 1.0]
G26_VOXEL = [0.125, 0.125, 0.25]                  # grid 64 x 48 x 8
G26_PFE = {
    'NAME': 'VoxelSetAbstraction', 'POINT_SOURCE': 'raw_points', 'NUM_KEYPOINTS': 48, 'NUM_OUTPUT_FEATURES': 16,
    'SAMPLE_METHOD': 'FPS', 'FEATURES_SOURCE': ['bev', 'x_conv1', 'x_conv2', 'x_conv3', 'x_conv4', 'raw_points'],
    'SA_LAYER': {
        'raw_points': {'MLPS': [[4, 4], [4, 4]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [4, 8]},
        'x_conv1': {'DOWNSAMPLE_FACTOR': 1, 'MLPS': [[4, 4], [4, 4]], 'POOL_RADIUS': [0.4, 0.8], 'NSAMPLE': [4, 8]},
        'x_conv2': {'DOWNSAMPLE_FACTOR': 2, 'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.8, 1.2], 'NSAMPLE': [4, 8]},
        'x_conv3': {'DOWNSAMPLE_FACTOR': 4, 'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [1.2, 2.4], 'NSAMPLE': [4, 8]},
        'x_conv4': {'DOWNSAMPLE_FACTOR': 8, 'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [2.4, 4.8], 'NSAMPLE': [4, 8]},
    },
}
G26_LEVEL_CHANNELS = {'x_conv1': 4, 'x_conv2': 8, 'x_conv3': 8, 'x_conv4': 8}   # = MLPS[0][0], the reference's rule
G26_BEV, G26_BEV_STRIDE = (8, 12, 16), 4           # C, H, W: a 16 x 12 map
G26_POINT_HEAD = {'NAME': 'PointHeadSimple', 'CLS_FC': [16, 16], 'CLASS_AGNOSTIC': True,
                  'USE_POINT_FEATURES_BEFORE_FUSION': True, 'TARGET_CONFIG': {'GT_EXTRA_WIDTH': [0.2, 0.2, 0.2]},
                  'LOSS_CONFIG': {'LOSS_REG': 'smooth-l1', 'LOSS_WEIGHTS': {'point_cls_weight': 1.0}}}
G26_ROI_HEAD = {
    'NAME': 'PVRCNNHead', 'CLASS_AGNOSTIC': True, 'SHARED_FC': [16, 16], 'CLS_FC': [16, 16], 'REG_FC': [16, 16],
    'DP_RATIO': 0.3,
    'NMS_CONFIG': {'TEST': {'NMS_TYPE': 'nms_gpu', 'MULTI_CLASSES_NMS': False, 'NMS_PRE_MAXSIZE': 64,
                            'NMS_POST_MAXSIZE': 6, 'NMS_THRESH': 0.7}},
    'ROI_GRID_POOL': {'GRID_SIZE': 2, 'MLPS': [[8, 8], [8, 8]], 'POOL_RADIUS': [0.8, 1.6], 'NSAMPLE': [4, 8],
                      'POOL_METHOD': 'max_pool'},
    'TARGET_CONFIG': {'BOX_CODER': 'ResidualCoder', 'ROI_PER_IMAGE': 6, 'FG_RATIO': 0.5, 'SAMPLE_ROI_BY_EACH_CLASS': True,
                      'CLS_SCORE_TYPE': 'roi_iou', 'CLS_FG_THRESH': 0.75, 'CLS_BG_THRESH': 0.25, 'CLS_BG_THRESH_LO': 0.1,
                      'HARD_BG_RATIO': 0.8, 'REG_FG_THRESH': 0.55},
    'LOSS_CONFIG': {'CLS_LOSS': 'BinaryCrossEntropy', 'REG_LOSS': 'smooth-l1', 'CORNER_LOSS_REGULARIZATION': True,
                    'LOSS_WEIGHTS': {'rcnn_cls_weight': 1.0, 'rcnn_reg_weight': 1.0, 'rcnn_corner_weight': 1.0,
                                     'code_weights': [1.0] * 7}},
}
G26_ROIS = 6


def sqdist(a, b):
    """(a.x-b.x)*(a.x-b.x) + (a.y-b.y)*(a.y-b.y) + (a.z-b.z)*(a.z-b.z), float32, left to right."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
    with np.errstate(all='ignore'):
        return (dx * dx + dy * dy) + dz * dz


def counts(column, B):
    """column (rows,) float32 or int32 -> cnt int32 (B), start int32 (B + 1), status bits."""
    column = np.asarray(column)
    cnt, st = np.zeros(B, np.int32), 0
    for r, v in enumerate(column):
        if 0 <= v < B and int(v) == v:
            cnt[int(v)] += 1
        else:
            st |= ST_BAD_BATCH
        if r + 1 < len(column) and column[r + 1] < v:
            st |= ST_UNSORTED
    return cnt, starts(cnt), st


def starts(cnt):
    out = np.zeros(len(cnt) + 1, np.int32)
    out[1:] = np.cumsum(np.maximum(np.asarray(cnt, np.int64), 0))
    return out


def fps_one(xyz, npoint):
    """xyz (n, 3), n >= 1 -> int32 (npoint <= n): first pick 0, running minimum from 1e10, then the largest running minimum,
    the lowest index among equals."""
    xyz = np.asarray(xyz, F32)
    idx = np.zeros(npoint, np.int32)
    run = np.full(len(xyz), 1e10, F32)
    old = 0
    for s in range(1, npoint):
        d = sqdist(xyz, xyz[old])
        with np.errstate(invalid='ignore'):
            run = np.where(d < run, d, run)
        old = int(np.argmax(run))
        idx[s] = old
    return idx


def fps(xyz, start, K):
    """xyz (N, 3) stacked -> idx int32 (B, K) sample-local, keypoints (B * K, 4), status.  A short sample cycles its picks;
    an empty one writes index 0, a zero keypoint and ST_EMPTY."""
    xyz = np.asarray(xyz, F32)
    B = len(start) - 1
    idx, kp, st = np.zeros((B, K), np.int32), np.zeros((B * K, 4), F32), 0
    for b in range(B):
        lo, n = int(start[b]), int(start[b + 1] - start[b])
        kp[b * K:(b + 1) * K, 0] = b
        if n == 0:
            st |= ST_EMPTY
            continue
        picks = fps_one(xyz[lo:lo + n], min(n, K))
        for j in range(K):
            idx[b, j] = picks[j % len(picks)]
        kp[b * K:(b + 1) * K, 1:] = xyz[lo + idx[b].astype(np.int64)]
    return idx, kp, st


def sample_of(start, m):
    for b in range(len(start) - 1):
        if start[b] <= m < start[b + 1]:
            return b
    return -1


def ball_query(xyz, start, centres, cstart, radius, nsample):
    """-> idx int32 (M, nsample) sample-local: the first nsample indices, ascending, with d2 < radius * radius (strict,
    float32) among the centre's own sample; the rest the first hit; zeros and empty = 1 without one."""
    xyz, centres = np.asarray(xyz, F32).reshape(-1, 3), np.asarray(centres, F32).reshape(-1, 3)
    M = len(centres)
    r2 = F32(radius) * F32(radius)
    idx, empty = np.zeros((M, nsample), np.int32), np.ones(M, np.uint8)
    for m in range(M):
        b = sample_of(cstart, m)
        if b < 0:
            continue
        lo, hi = int(start[b]), int(start[b + 1])
        with np.errstate(invalid='ignore'):
            hits = np.nonzero(sqdist(centres[m], xyz[lo:hi]) < r2)[0][:nsample]   # the walk stops at nsample hits
        if len(hits):
            idx[m, :] = hits[0]
            idx[m, :len(hits)] = hits
            empty[m] = 0
    return idx, empty


def group(xyz, start, centres, cstart, features, idx, empty):
    """-> (3 + C, M, nsample): xyz[start_b + idx] - centre, then the feature row (bits); empty balls zeros."""
    xyz, centres = np.asarray(xyz, F32).reshape(-1, 3), np.asarray(centres, F32).reshape(-1, 3)
    M, ns = idx.shape
    C = 0 if features is None else features.shape[1]
    out = np.zeros((3 + C, M, ns), F32)
    bits = out.view(np.uint32)
    for m in range(M):
        if empty[m]:
            continue
        lo = int(start[sample_of(cstart, m)])
        for j in range(ns):
            g = lo + int(idx[m, j])
            out[0:3, m, j] = xyz[g] - centres[m]
            if C:
                bits[3:, m, j] = features[g].view(np.uint32)
    return out


def group_backward(grad_out, start, cstart, idx, empty, N):
    """grad_out (3 + C, M, nsample) -> (N, C): per source row the entries in ascending entry number, one float32 addition
    each, from +0.0."""
    C, (M, ns) = grad_out.shape[0] - 3, idx.shape
    gf = np.zeros((N, C), F32)
    for m in range(M):
        if empty[m]:
            continue
        lo = int(start[sample_of(cstart, m)])
        for j in range(ns):
            g = lo + int(idx[m, j])
            gf[g] = gf[g] + grad_out[3:, m, j]
    return gf


def bev_sample(keypoints, spatial, pc_range, voxel_size, bev_stride):
    """keypoints (M, 4), spatial (B, C, H, W) -> (M, C); the reference's arithmetic in float32."""
    kp, sp = np.asarray(keypoints, F32), np.asarray(spatial, F32)
    B, C, H, W = sp.shape
    out = np.zeros((len(kp), C), F32)
    with np.errstate(all='ignore'):
        fx = ((kp[:, 1] - F32(pc_range[0])) / F32(voxel_size[0])) / F32(bev_stride)
        fy = ((kp[:, 2] - F32(pc_range[1])) / F32(voxel_size[1])) / F32(bev_stride)
    for m in range(len(kp)):
        b = int(kp[m, 0])
        x, y = fx[m], fy[m]
        x0 = int(np.floor(x))
        y0 = int(np.floor(y))
        x1, y1 = x0 + 1, y0 + 1
        x0, x1 = min(max(x0, 0), W - 1), min(max(x1, 0), W - 1)
        y0, y1 = min(max(y0, 0), H - 1), min(max(y1, 0), H - 1)
        Ia, Ib, Ic, Id = sp[b, :, y0, x0], sp[b, :, y1, x0], sp[b, :, y0, x1], sp[b, :, y1, x1]
        wa = (F32(x1) - x) * (F32(y1) - y)
        wb = (F32(x1) - x) * (y - F32(y0))
        wc = (x - F32(x0)) * (F32(y1) - y)
        wd = (x - F32(x0)) * (y - F32(y0))
        out[m] = ((Ia * wa + Ib * wb) + Ic * wc) + Id * wd
    return out


def stacked_cloud(seed, counts_, scale=2.0):
    """rows of all samples, float32 (sum, 3), from a continuous distribution, and its start array."""
    n = int(sum(counts_))
    return (np.random.default_rng(seed).normal(0.0, 1.0, (n, 3)) * scale).astype(F32), starts(counts_)
