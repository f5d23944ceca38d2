"""NumPy restatement of SURVEY.md §8 row f-10: OpenPCDet's world augmentation (random_world_flip / _rotation /
_scaling / _translation), the heading wrap, the class filter with its class column, mask_points_and_boxes_outside_range
and collate_batch, with the values the reference would draw given as arguments.  It is what tests compare the HIP stage
against bit for bit, and what tests/test_oracle_world_aug.py compares with the reference's own run (golden G15).

One thing is DEFINED here rather than copied: the rotation.  The reference's float32 matmul gives different bits for
different row counts; this restatement and the stage use the chain it gives from 64 rows on,
x' = fma(y, -s, x*c), y' = fma(y, c, x*s), z' = z, and a zero result is +0 (the matmul accumulates onto +0).
"""
import numpy as np
import torch

from dfu3d_amd.calibration import fma_f32

TWO_PI_F = np.float32(2 * np.pi)


def cos_sin_f32(noise_rot):
    """cos and sin of the angle as rotate_points_along_z forms them: the float64 angle cast to float32, torch's float32
    cos / sin."""
    a = torch.from_numpy(np.array([noise_rot])).float()
    return np.float32(torch.cos(a).numpy()[0]), np.float32(torch.sin(a).numpy()[0])


def rot_z(xyz, c, s):
    """(n, 3) -> (n, 3) float32 by the defined chain."""
    xyz = np.asarray(xyz).astype(np.float32)
    x, y = xyz[:, 0], xyz[:, 1]
    out = xyz.copy()
    if len(xyz):
        out[:, 0] = fma_f32(y, np.broadcast_to(-s, y.shape), x * c)
        out[:, 1] = fma_f32(y, np.broadcast_to(c, y.shape), x * s)
    return out + np.float32(0.0)                     # -0 -> +0, nothing else changes


def limit_period_f32(h):
    h = np.asarray(h).astype(np.float32)
    return h - np.floor(h / TWO_PI_F + np.float32(0.5)) * TWO_PI_F


def augment(points, boxes, drawn):
    """One scene.  points (n, C) float32, boxes (m, 7|9) float32 or float64; drawn: {'flips': [(axis, bool), ...] in
    ALONG_AXIS_LIST order, 'noise_rot': float or None, 'noise_scale': float or None, 'noise_translate': float32 (1, 3) or
    None, 'wrap': bool (default True)} -> (points, boxes, steps): new arrays, and the arrays after every step by name."""
    p, b = points.copy(), boxes.copy()
    steps = {}
    for axis, on in drawn.get('flips', []):
        if on and axis == 'x':
            p[:, 1] = -p[:, 1]
            b[:, 1] = -b[:, 1]
            b[:, 6] = -b[:, 6]
            if b.shape[1] > 7:
                b[:, 8] = -b[:, 8]
        elif on:
            p[:, 0] = -p[:, 0]
            b[:, 0] = -b[:, 0]
            b[:, 6] = -(b[:, 6] + b.dtype.type(np.pi))
            if b.shape[1] > 7:
                b[:, 7] = -b[:, 7]
    steps['flip'] = (p.copy(), b.copy())
    if drawn.get('noise_rot') is not None:
        rot = drawn['noise_rot']
        c, s = cos_sin_f32(rot)
        p[:, 0:3] = rot_z(p[:, 0:3], c, s)
        b[:, 0:3] = rot_z(b[:, 0:3], c, s)
        b[:, 6] += b.dtype.type(rot)
        if b.shape[1] > 7:
            v = np.concatenate([b[:, 7:9], np.zeros((len(b), 1), b.dtype)], 1)
            b[:, 7:9] = rot_z(v, c, s)[:, 0:2]
    steps['rotation'] = (p.copy(), b.copy())
    if drawn.get('noise_scale') is not None:
        sc = drawn['noise_scale']
        p[:, 0:3] *= np.float32(sc)
        b[:, 0:6] *= b.dtype.type(sc)
        if b.shape[1] > 7:
            b[:, 7:] *= b.dtype.type(sc)
    steps['scaling'] = (p.copy(), b.copy())
    if drawn.get('noise_translate') is not None:
        t = np.asarray(drawn['noise_translate'], np.float32).reshape(1, 3)
        p[:, 0:3] += t
        b[:, 0:3] += t.astype(b.dtype)
    steps['translation'] = (p.copy(), b.copy())
    if drawn.get('wrap', True):
        b[:, 6] = limit_period_f32(b[:, 6]).astype(b.dtype)
    return p, b, steps


def class_ids(names, class_names):
    """1-based index into class_names, 0 for a name that is not there."""
    class_names = list(class_names)
    return np.array([class_names.index(n) + 1 if n in class_names else 0 for n in names], np.int32)


def class_filter(boxes, cls):
    """dataset.py:194-200: the rows whose class is known, with the class id as a float32 column (the result keeps the
    boxes' dtype, as np.concatenate gives it)."""
    sel = cls > 0
    return np.concatenate([boxes[sel], cls[sel].reshape(-1, 1).astype(np.float32)], 1), sel


def point_mask(points, pc_range):
    r = np.asarray(pc_range, np.float32)
    return (points[:, 0] >= r[0]) & (points[:, 0] <= r[3]) & (points[:, 1] >= r[1]) & (points[:, 1] <= r[4])


def box_mask(boxes, pc_range):
    r = np.asarray(pc_range, np.float32)
    c = boxes[:, 0:3]
    return ((c >= r[0:3]) & (c <= r[3:6])).all(axis=-1)


def scene(points, boxes, cls, drawn, pc_range, mask_points=True, mask_boxes=True, filter_class=True):
    """One scene from the sampler's output to what collate_batch gets: (points (k, C), gt_boxes (j, 8|10), kept box rows)."""
    p, b, _ = augment(points, boxes, drawn)
    keep = np.ones(len(b), bool)
    if filter_class:
        keep &= cls > 0
    if mask_boxes:
        keep &= box_mask(b, pc_range)
    g = np.concatenate([b[keep], cls[keep].reshape(-1, 1).astype(np.float32)], 1)
    if mask_points:
        p = p[point_mask(p, pc_range)]
    return p, g, keep


def collate(points_list, boxes_list):
    """dataset.py collate_batch for `points` and `gt_boxes`."""
    C = points_list[0].shape[1]
    pts = [np.pad(p, ((0, 0), (1, 0)), mode='constant', constant_values=i) for i, p in enumerate(points_list)]
    pts = np.concatenate(pts, 0).astype(np.float32) if pts else np.zeros((0, C + 1), np.float32)
    max_gt = max(len(x) for x in boxes_list)
    gt = np.zeros((len(boxes_list), max_gt, boxes_list[0].shape[-1]), np.float32)
    for k, x in enumerate(boxes_list):
        gt[k, :len(x), :] = x
    return pts, gt


def batch(scenes, pc_range, mask_points=True, mask_boxes=True, filter_class=True):
    """scenes: [(points, boxes, cls, drawn), ...] -> (points (sum k, 1 + C), gt_boxes (B, max_gt, 8|10), point_cnt (B),
    gt_cnt (B)): what the stage returns, cut at n_kept and max(gt_cnt)."""
    ps, gs = [], []
    for points, boxes, cls, drawn in scenes:
        p, g, _ = scene(points, boxes, cls, drawn, pc_range, mask_points, mask_boxes, filter_class)
        ps.append(p)
        gs.append(g)
    pts, gt = collate(ps, gs)
    return pts, gt, np.array([len(p) for p in ps], np.int32), np.array([len(g) for g in gs], np.int32)
