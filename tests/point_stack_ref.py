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
    with np.errstate(all='ignore'):
        dx, dy, dz = a[..., 0] - b[..., 0], a[..., 1] - b[..., 1], a[..., 2] - b[..., 2]
        return (dx * dx + dy * dy) + dz * dz


def counts(column, B):
    """column (rows,) float32 or int32 -> cnt int32 (B), start int32 (B + 1), status bits."""
    column = np.asarray(column)
    with np.errstate(invalid='ignore'):
        good = (column >= 0) & (column < B) & (np.floor(column) == column)      # all False for a NaN
        unsorted = bool((column[1:] < column[:-1]).any())
    cnt = np.bincount(column[good].astype(np.int64), minlength=B).astype(np.int32)
    st = (0 if good.all() else ST_BAD_BATCH) | (ST_UNSORTED if unsorted else 0)
    return cnt, starts(cnt), st


def starts(cnt):
    out = np.zeros(len(cnt) + 1, np.int32)
    out[1:] = np.cumsum(np.maximum(np.asarray(cnt, np.int64), 0))
    return out


def starts_status(cnt):
    """The status of starts(): a negative count is taken as 0 and sets ST_BAD_COUNT."""
    return ST_BAD_COUNT if (np.asarray(cnt, np.int64) < 0).any() else 0


def sample_rows(start, b, rows):
    """The rows of sample b inside [0, rows] -> lo, n, status: start[b] clamped to [0, rows], start[b + 1] to [lo, rows];
    ST_BAD_COUNT when either moved."""
    a, e = int(start[b]), int(start[b + 1])
    lo = min(max(a, 0), rows)
    hi = lo if e < lo else min(e, rows)
    return lo, hi - lo, (ST_BAD_COUNT if (lo != a or hi != e) else 0)


def fps_one(xyz, npoint, ties=None):
    """xyz (n, 3), n >= 1 -> int32 (npoint <= n): first pick 0, running minimum from 1e10, then the largest running minimum,
    the lowest index among equals.  ties: a list that receives every step with more than one candidate at the maximum."""
    xyz = np.asarray(xyz, F32)
    idx = np.zeros(npoint, np.int32)
    run = np.full(len(xyz), 1e10, F32)
    old = 0
    for s in range(1, npoint):
        d = sqdist(xyz, xyz[old])
        with np.errstate(invalid='ignore'):
            run = np.where(d < run, d, run)
        old = int(np.argmax(run))
        if ties is not None and int((run == run[old]).sum()) > 1:
            ties.append(s)
        idx[s] = old
    return idx


def fps_plain64(xyz, npoint):
    """The same sampling in float64, written without the restatement's helpers: on coordinates whose differences, squares
    and sums are exact in float32 it is the restatement's picks index for index."""
    p = np.asarray(xyz, np.float64)
    run = np.full(len(p), 1e10)
    picks = [0]
    for _ in range(1, npoint):
        q = p[picks[-1]]
        run = np.minimum(run, ((p - q) ** 2).sum(axis=1))
        picks.append(int(np.flatnonzero(run == run.max())[0]))
    return np.asarray(picks, np.int32)


def fps_bound(rows, cap):
    """The bound on a sample: cap if 1 <= cap < rows, else rows."""
    return cap if 1 <= cap < rows else rows


def fps(xyz, start, K, cap=0, rows=None):
    """xyz (N, 3) stacked -> idx int32 (B, K) sample-local, keypoints (B * K, 4), status.  A short sample cycles its picks;
    an empty one writes index 0, a zero keypoint and ST_EMPTY.  rows: the rows the call is told of (default: all of xyz);
    starts are clamped as sample_rows states.  A sample beyond fps_bound(rows, cap) is cut to its first `bound` rows and
    sets ST_BAD_COUNT.  A non-finite coordinate among the sampled rows sets ST_BAD_POINT: the picks returned for that
    sample are then NOT specified (only that they lie inside the sample)."""
    xyz = np.asarray(xyz, F32)
    rows = len(xyz) if rows is None else int(rows)
    bound = fps_bound(rows, int(cap))
    B = len(start) - 1
    idx, kp, st = np.zeros((B, K), np.int32), np.zeros((B * K, 4), F32), 0
    for b in range(B):
        lo, n, bad = sample_rows(start, b, rows)
        st |= bad
        if n > bound:
            st |= ST_BAD_COUNT
            n = bound
        kp[b * K:(b + 1) * K, 0] = b
        if n == 0:
            st |= ST_EMPTY
            continue
        if not np.isfinite(xyz[lo:lo + n]).all():
            st |= ST_BAD_POINT
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


def centre_rows(start, cstart, m, N):
    """The rows of the sample of centre m -> lo, n, status: sample_rows of the sample whose centres hold m; a centre at or
    beyond cstart[B] has no sample: no rows and ST_BAD_COUNT."""
    b = sample_of(cstart, m)
    return (0, 0, ST_BAD_COUNT) if b < 0 else sample_rows(start, b, N)


def ball_query(xyz, start, centres, cstart, radius, nsample, with_status=False):
    """-> idx int32 (M, nsample) sample-local: the first nsample indices, ascending, with d2 < radius * radius (strict,
    float32) among the centre's own sample; the rest the first hit; zeros and empty = 1 without one.  Starts are clamped
    to the rows of xyz as sample_rows states; a centre beyond cstart[B] is an empty ball and sets ST_BAD_COUNT.
    with_status: the status bits as a third result."""
    xyz, centres = np.asarray(xyz, F32).reshape(-1, 3), np.asarray(centres, F32).reshape(-1, 3)
    M = len(centres)
    r2 = F32(radius) * F32(radius)
    idx, empty, st = np.zeros((M, nsample), np.int32), np.ones(M, np.uint8), 0
    for m in range(M):
        lo, n, bad = centre_rows(start, cstart, m, len(xyz))
        st |= bad
        with np.errstate(invalid='ignore'):
            hits = np.nonzero(sqdist(centres[m], xyz[lo:lo + n]) < r2)[0][:nsample]   # the walk stops at nsample hits
        if len(hits):
            idx[m, :] = hits[0]
            idx[m, :len(hits)] = hits
            empty[m] = 0
    return (idx, empty, st) if with_status else (idx, empty)


def group(xyz, start, centres, cstart, features, idx, empty, with_status=False):
    """-> (3 + C, M, nsample): xyz[start_b + idx] - centre, then the feature row (bits); empty balls zeros.  xyz and
    centres None: the plain form, (C, M, nsample).  Starts are clamped (over the rows of xyz, or of the features in the
    plain form); a centre beyond cstart[B] sets ST_BAD_COUNT; an index outside its sample (of a ball not marked empty) sets
    ST_BAD_INDEX and reads row 0 of the sample, zeros for a sample without rows."""
    plain = xyz is None
    if not plain:
        xyz, centres = np.asarray(xyz, F32).reshape(-1, 3), np.asarray(centres, F32).reshape(-1, 3)
    M, ns = idx.shape
    C = 0 if features is None else features.shape[1]
    N = len(features) if plain else len(xyz)
    xo = 0 if plain else 3
    out, st = np.zeros((xo + C, M, ns), F32), 0
    bits = out.view(np.uint32)
    for m in range(M):
        lo, n, bad = centre_rows(start, cstart, m, N)
        st |= bad
        if empty[m]:
            continue
        for j in range(ns):
            i = int(idx[m, j])
            if not 0 <= i < n:
                st |= ST_BAD_INDEX
                i = 0
                if n == 0:
                    continue
            g = lo + i
            if not plain:
                out[0:3, m, j] = xyz[g] - centres[m]
            if C:
                bits[xo:, m, j] = features[g].view(np.uint32)
    return (out, st) if with_status else out


def global_index(start, cstart, idx, empty, N):
    """-> gidx int32 (M * nsample), status: start_b + idx, -1 for the entries of an empty ball and for an index outside its
    sample (ST_BAD_INDEX); a centre beyond cstart[B] sets ST_BAD_COUNT, whether its ball is marked empty or not."""
    M, ns = idx.shape
    gidx, st = np.full((M, ns), -1, np.int32), 0
    for m in range(M):
        lo, n, bad = centre_rows(start, cstart, m, N)
        st |= bad
        if empty[m]:
            continue
        for j in range(ns):
            i = int(idx[m, j])
            if 0 <= i < n:
                gidx[m, j] = lo + i
            else:
                st |= ST_BAD_INDEX
    return gidx.reshape(-1), st


def group_backward(grad_out, start, cstart, idx, empty, N, with_status=False, skip=3):
    """grad_out (skip + C, M, nsample) -> (N, C): per source row the entries in ascending entry number, one float32
    addition each, from +0.0; the entries global_index marks -1 are left out."""
    C, (M, ns) = grad_out.shape[0] - skip, idx.shape
    gidx, st = global_index(start, cstart, idx, empty, N)
    gf = np.zeros((N, C), F32)
    flat = grad_out[skip:].reshape(C, M * ns)
    for e in np.flatnonzero(gidx >= 0):
        gf[gidx[e]] = gf[gidx[e]] + flat[:, e]
    return (gf, st) if with_status else gf


def clamp_floor(f, hi):
    """floor(f) (an integral float) clamped to [0, hi]; NaN and both infinities give 0, as the reference's
    torch.floor(x).long() followed by torch.clamp(x0, 0, hi) does on the host, where the conversion of a non-finite float
    is the most negative int64 -- and so is that value + 1."""
    if not np.isfinite(f):
        return 0
    return int(min(max(f, F32(0.0)), F32(hi)))


def bev_sample(keypoints, spatial, pc_range, voxel_size, bev_stride, with_status=False):
    """keypoints (M, 4), spatial (B, C, H, W) -> (M, C); the reference's arithmetic in float32.  A sample index outside
    [0, B) or not an integer: a row of zeros and ST_BAD_BATCH.  A non-finite map coordinate takes index 0 on its axis for
    both neighbours (clamp_floor)."""
    kp, sp = np.asarray(keypoints, F32), np.asarray(spatial, F32)
    B, C, H, W = sp.shape
    out, st = np.zeros((len(kp), C), F32), 0
    with np.errstate(all='ignore'):
        fx = ((kp[:, 1] - F32(pc_range[0])) / F32(voxel_size[0])) / F32(bev_stride)
        fy = ((kp[:, 2] - F32(pc_range[1])) / F32(voxel_size[1])) / F32(bev_stride)
        for m in range(len(kp)):
            fb = kp[m, 0]
            if not (fb >= 0 and fb < B and np.floor(fb) == fb):
                st |= ST_BAD_BATCH
                continue
            b = int(fb)
            x, y = fx[m], fy[m]
            flx, fly = np.floor(x), np.floor(y)
            x0, x1 = clamp_floor(flx, W - 1), clamp_floor(flx + F32(1.0), W - 1)
            y0, y1 = clamp_floor(fly, H - 1), clamp_floor(fly + F32(1.0), H - 1)
            Ia, Ib, Ic, Id = sp[b, :, y0, x0], sp[b, :, y1, x0], sp[b, :, y0, x1], sp[b, :, y1, x1]
            wa = (F32(x1) - x) * (F32(y1) - y)
            wb = (F32(x1) - x) * (y - F32(y0))
            wc = (x - F32(x0)) * (F32(y1) - y)
            wd = (x - F32(x0)) * (y - F32(y0))
            out[m] = ((Ia * wa + Ib * wb) + Ic * wc) + Id * wd
    return (out, st) if with_status else out


def same_bits_or_nan(a, b):
    """Bit equality, except that any NaN equals any NaN: IEEE 754 leaves the sign and payload of the NaN an invalid
    operation (inf - inf, 0 * inf) makes to the implementation, and a processor and NumPy differ in them."""
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool((na == nb).all() and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def lattice_cloud(seed, counts_, pitch=0.25, span=2):
    """rows of all samples, float32 (sum, 3), and its start array: integer multiples of `pitch` in [-span, span] * pitch on
    every axis, so that with a pitch that is a power of two and a small span every float32 subtraction, square and sum of a
    squared distance is exact (pitch 0.25, span 2: multiples of 1/16 up to 3).  (2 * span + 1) ** 3 cells: a sample with
    more rows than that has duplicates, and the maxima of farthest point sampling tie."""
    n = int(sum(counts_))
    cells = np.random.default_rng(seed).integers(-span, span + 1, (n, 3))
    return (cells * pitch).astype(F32), starts(counts_)


def stacked_cloud(seed, counts_, scale=2.0):
    """rows of all samples, float32 (sum, 3), from a continuous distribution, and its start array."""
    n = int(sum(counts_))
    return (np.random.default_rng(seed).normal(0.0, 1.0, (n, 3)) * scale).astype(F32), starts(counts_)
