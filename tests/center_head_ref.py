"""CPU restatement (NumPy) of the CenterHead geometry of row f-6: `CenterHead.assign_targets`
(pcdet/models/dense_heads/center_head.py:106-227) and `decode_bbox_from_heatmap`
(pcdet/models/model_utils/centernet_utils.py:155-241), in the reference's float32 operation order.  Golden G12
(tests/golden/capture_center_head_golden.py) pins it on the reference's own run; the GPU tests compare the kernels with
it on inputs the golden does not hold.  Transcendentals (log, cos, sin, atan2) and the Gaussian are evaluated in fp64 and
rounded to float32, as the kernels do.

Stated divergence from the reference: boxes are assigned by the caller's ORIGINAL class ids and `gt_boxes` is not
written (the reference rewrites the class column head by head and looks the names up again from the rewritten column).
"""
import numpy as np

f32 = np.float32

CFG_A = dict(
    class_names=['Car', 'Truck', 'Construction_vehicle', 'Bus', 'Trailer', 'Barrier', 'Motorcycle', 'Bicycle',
                 'Pedestrian', 'Traffic_cone'],
    heads=[['Car'], ['Truck', 'Construction_vehicle'], ['Bus', 'Trailer'], ['Barrier'], ['Motorcycle', 'Bicycle'],
           ['Pedestrian', 'Traffic_cone']],
    point_cloud_range=[0, -51.2, -5.0, 51.2, 51.2, 3.0], voxel_size=[0.2, 0.2, 8.0], stride=4, map_hw=(128, 64),
    num_max_objs=500, gaussian_overlap=0.1, min_radius=2, C=8)
CFG_B = dict(
    class_names=['Car', 'Pedestrian', 'Cyclist'], heads=[['Car'], ['Pedestrian', 'Cyclist']],
    point_cloud_range=[0, -40.0, -3.0, 70.4, 40.0, 1.0], voxel_size=[0.1, 0.1, 0.15], stride=8, map_hw=(100, 88),
    num_max_objs=8, gaussian_overlap=0.1, min_radius=2, C=10)


def head_tables(class_names, heads):
    """cls_tab (n_cls + 1, 2): class id -> (head, 0-based id within the head), row 0 = (-1, -1); head_plane (n_heads + 1)."""
    tab = -np.ones((len(class_names) + 1, 2), np.int32)
    plane = [0]
    for h, names in enumerate(heads):
        names = [n for n in names if n in class_names]
        for j, n in enumerate(names):
            tab[class_names.index(n) + 1] = (h, j)
        plane.append(plane[-1] + len(names))
    return tab, np.asarray(plane, np.int32)


def gaussian_radius(height, width, min_overlap):
    """centernet_utils.py:9-35 on float32 arrays: every Python scalar is rounded to float32 once, as torch does."""
    o = min_overlap
    k1, k2, a34, b3k, c3k = f32(1 - o), f32(1 + o), f32(4 * (4 * o)), f32(-2 * o), f32(o - 1)
    b1 = height + width
    c1 = width * height * k1 / k2
    r1 = (b1 + np.sqrt(b1 * b1 - f32(4) * c1)) / f32(2)
    b2 = f32(2) * b1
    c2 = k1 * width * height
    r2 = (b2 + np.sqrt(b2 * b2 - f32(16) * c2)) / f32(2)
    b3 = b3k * b1
    c3 = c3k * width * height
    r3 = (b3 + np.sqrt(b3 * b3 - a34 * c3)) / f32(2)
    return np.minimum(np.minimum(r1, r2), r3)


def gaussian2d(radius):
    """centernet_utils.py:38-44 for shape (2r + 1, 2r + 1), sigma = (2r + 1) / 6: fp64."""
    sigma = (2 * radius + 1) / 6
    y, x = np.ogrid[-radius:radius + 1, -radius:radius + 1]
    y, x = y.astype(np.float64), x.astype(np.float64)
    h = np.exp(-(x * x + y * y) / (2 * sigma * sigma))
    h[h < np.finfo(np.float64).eps * h.max()] = 0
    return h


def _round_f64(fn, v):
    return fn(np.asarray(v, np.float64)).astype(f32)


def assign_targets(gt_boxes, cfg, map_hw=None):
    """gt_boxes float32 (B, M, C) -> dict of per-head lists like the reference's ret_dict, plus 'draws': per head an
    int array (n, 4) of (sample, cx, cy, radius) in slot order.  Raises RuntimeError where the reference does (more
    than num_max_objs boxes of one head in one sample)."""
    gt_boxes = np.ascontiguousarray(gt_boxes, f32)
    B, M, C = gt_boxes.shape
    H, W = map_hw if map_hw is not None else cfg['map_hw']
    tab, plane = head_tables(cfg['class_names'], cfg['heads'])
    nmax, stride = cfg['num_max_objs'], f32(cfg['stride'])
    rx, ry = f32(cfg['point_cloud_range'][0]), f32(cfg['point_cloud_range'][1])
    vx, vy = f32(cfg['voxel_size'][0]), f32(cfg['voxel_size'][1])
    n_heads = len(plane) - 1
    ret = {k: [] for k in ('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src', 'draws')}
    ret['heatmap_masks'] = []
    cls = gt_boxes[..., -1].astype(np.int64)
    ok = (cls >= 1) & (cls < len(tab))
    head_of = np.where(ok, tab[np.where(ok, cls, 0), 0], -1)
    local_of = np.where(ok, tab[np.where(ok, cls, 0), 1], -1)
    for h in range(n_heads):
        ncls = int(plane[h + 1] - plane[h])
        hm = np.zeros((B, ncls, H, W), f32)
        tb = np.zeros((B, nmax, C), f32)
        src = np.zeros((B, nmax, C), f32)
        inds = np.zeros((B, nmax), np.int64)
        masks = np.zeros((B, nmax), np.int64)
        draws = []
        for b in range(B):
            rows = np.nonzero(head_of[b] == h)[0]
            if len(rows) > nmax:
                raise RuntimeError('head %d, sample %d: %d boxes, NUM_MAX_OBJS = %d' % (h, b, len(rows), nmax))
            g = gt_boxes[b, rows].copy()
            g[:, -1] = (local_of[b, rows] + 1).astype(f32)
            n = len(rows)
            src[b, :n] = g
            cx = np.clip((g[:, 0] - rx) / vx / stride, f32(0), f32(W - 0.5))
            cy = np.clip((g[:, 1] - ry) / vy / stride, f32(0), f32(H - 0.5))
            cxi, cyi = cx.astype(np.int32), cy.astype(np.int32)
            dx, dy = g[:, 3] / vx / stride, g[:, 4] / vy / stride
            with np.errstate(invalid='ignore'):
                rad = gaussian_radius(dx, dy, cfg['gaussian_overlap'])
            for k in range(n):
                if dx[k] <= 0 or dy[k] <= 0:
                    continue
                r = max(int(rad[k]), cfg['min_radius'])
                x, y = int(cxi[k]), int(cyi[k])
                gauss = gaussian2d(r)
                left, right = min(x, r), min(W - x, r + 1)
                top, bottom = min(y, r), min(H - y, r + 1)
                view = hm[b, int(g[k, -1]) - 1, y - top:y + bottom, x - left:x + right]
                np.maximum(view, gauss[r - top:r + bottom, r - left:r + right].astype(f32), out=view)
                draws.append((b, x, y, r))
                inds[b, k] = y * W + x
                masks[b, k] = 1
                tb[b, k, 0] = cx[k] - f32(cxi[k])
                tb[b, k, 1] = cy[k] - f32(cyi[k])
                tb[b, k, 2] = g[k, 2]
                tb[b, k, 3:6] = _round_f64(np.log, g[k, 3:6])
                tb[b, k, 6] = _round_f64(np.cos, g[k, 6])
                tb[b, k, 7] = _round_f64(np.sin, g[k, 6])
                if C > 8:
                    tb[b, k, 8:] = g[k, 7:-1]
        ret['heatmaps'].append(hm)
        ret['target_boxes'].append(tb)
        ret['inds'].append(inds)
        ret['masks'].append(masks)
        ret['target_boxes_src'].append(src)
        ret['draws'].append(np.asarray(draws, np.int32).reshape(-1, 4))
    return ret


def score_keys(flat):
    """Monotone uint32 key of torch.topk's order: NaN above every number, -0 == +0."""
    flat = np.ascontiguousarray(flat, f32)
    b = flat.view(np.uint32).copy()
    b[b == np.uint32(0x80000000)] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(flat)] = np.uint32(0xFFFFFFFF)
    return key


def decode_bbox_from_heatmap(heatmap, rot_cos, rot_sin, center, center_z, dim, point_cloud_range, voxel_size,
                             feature_map_stride, vel=None, iou=None, K=100, score_thresh=None,
                             post_center_limit_range=None):
    """The stated rule: the K best of a sample by descending score, ties by ascending flat index class * H * W + cell."""
    B, n_cls, H, W = heatmap.shape
    HW = H * W
    if K > n_cls * HW:
        raise RuntimeError('K = %d exceeds the %d scores of a sample' % (K, n_cls * HW))
    stride = f32(feature_map_stride)
    rx, ry = f32(point_cloud_range[0]), f32(point_cloud_range[1])
    vx, vy = f32(voxel_size[0]), f32(voxel_size[1])
    lim = np.asarray(post_center_limit_range, f32)
    out = []
    for b in range(B):
        flat = np.ascontiguousarray(heatmap[b], f32).reshape(-1)
        key = score_keys(flat).astype(np.int64)
        order = np.lexsort((np.arange(flat.size), -key))[:K]
        cls, cell = order // HW, order % HW
        ys, xs = (cell // W).astype(f32), (cell % W).astype(f32)
        g = lambda m, c: np.ascontiguousarray(m[b, c], f32).reshape(-1)[cell]   # noqa: E731
        bx = [(xs + g(center, 0)) * stride * vx + rx, (ys + g(center, 1)) * stride * vy + ry, g(center_z, 0),
              g(dim, 0), g(dim, 1), g(dim, 2),
              np.arctan2(g(rot_sin, 0).astype(np.float64), g(rot_cos, 0).astype(np.float64)).astype(f32)]
        if vel is not None:
            bx += [g(vel, 0), g(vel, 1)]
        boxes = np.stack(bx, axis=1).astype(f32)
        scores = flat[order]
        mask = (boxes[:, :3] >= lim[:3]).all(1) & (boxes[:, :3] <= lim[3:]).all(1)
        if score_thresh is not None:
            mask &= scores > f32(score_thresh)
        d = {'pred_boxes': boxes[mask], 'pred_scores': scores[mask], 'pred_labels': cls[mask].astype(np.int32),
             'order': order[mask]}
        if iou is not None:
            d['pred_iou'] = g(iou, 0)[mask]
        out.append(d)
    return out


def decode_inputs(seed, B, n_cls, H, W, with_vel, with_iou):
    """Heat maps with provably distinct scores, (perm + 1) / (N + 1) over a permutation of the N cells of a sample, and
    random regression maps, from NumPy's frozen legacy stream (np.random.RandomState)."""
    rs = np.random.RandomState(seed)
    N = n_cls * H * W
    heat = np.stack([((rs.permutation(N) + 1) / (N + 1)).astype(f32) for _ in range(B)]).reshape(B, n_cls, H, W)
    d = {'heatmap': heat,
         'center': rs.uniform(-0.5, 1.5, (B, 2, H, W)).astype(f32),
         'center_z': rs.uniform(-12, 12, (B, 1, H, W)).astype(f32),
         'dim': rs.uniform(0.3, 6, (B, 3, H, W)).astype(f32),
         'rot_cos': rs.uniform(-1, 1, (B, 1, H, W)).astype(f32),
         'rot_sin': rs.uniform(-1, 1, (B, 1, H, W)).astype(f32),
         'vel': rs.uniform(-5, 5, (B, 2, H, W)).astype(f32) if with_vel else None,
         'iou': rs.uniform(0, 1, (B, 1, H, W)).astype(f32) if with_iou else None}
    for b in range(B):
        assert np.unique(heat[b]).size == N
    return d


def ulp_diff(a, b):
    """Distance in float32 steps between two float32 arrays (finite values, or equal infinities)."""
    def lin(v):
        i = np.ascontiguousarray(v, f32).view(np.int32).astype(np.int64)
        return np.where(i < 0, np.int64(-2 ** 31) - i, i)
    return np.abs(lin(a) - lin(b))
