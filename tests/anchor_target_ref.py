"""NumPy float32 restatement of the reference's anchor target assignment (AxisAlignedTargetAssigner.assign_targets for
POS_FRACTION < 0, NORM_BY_NUM_EXAMPLES False, MATCH_HEIGHT False, no multihead): the loop over samples and anchor
classes, the dense (anchors x boxes) nearest-BEV IoU matrix operation by operation, the two arg maxima, the forced
anchors, the labels, ResidualCoder.encode_torch.  It shares no code with the package's modules.

Also here, because the host test checks them on the CPU with this restatement and the GPU test runs them: the class sets
of cfgs/kitti_models/second_ps.yaml, the anchors of a feature map, the fixture shapes of golden G25 and the CASES of
tests/test_gpu_anchor_target.py, each asserting that the condition it is named after occurs."""
import math

import numpy as np

F = np.float32
PI = F(np.pi)
QUARTER = F(np.pi / 4)

CLASS_NAMES = ['Car', 'Pedestrian', 'Bicycle']
# ANCHOR_GENERATOR_CONFIG of second_ps.yaml
ANCHOR_CFG = [
    {'class_name': 'Car', 'anchor_sizes': [[3.9, 1.6, 1.56]], 'anchor_rotations': [0, 1.57], 'anchor_bottom_heights': [-1.78],
     'align_center': False, 'feature_map_stride': 8, 'matched_threshold': 0.6, 'unmatched_threshold': 0.45},
    {'class_name': 'Pedestrian', 'anchor_sizes': [[0.8, 0.6, 1.73]], 'anchor_rotations': [0, 1.57],
     'anchor_bottom_heights': [-0.6], 'align_center': False, 'feature_map_stride': 8, 'matched_threshold': 0.5,
     'unmatched_threshold': 0.35},
    {'class_name': 'Bicycle', 'anchor_sizes': [[1.76, 0.6, 1.73]], 'anchor_rotations': [0, 1.57],
     'anchor_bottom_heights': [-0.6], 'align_center': False, 'feature_map_stride': 8, 'matched_threshold': 0.5,
     'unmatched_threshold': 0.35},
]
# the dense head of second_ps.yaml
HEAD_CFG = {
    'NAME': 'AnchorHeadSingle', 'CLASS_AGNOSTIC': False, 'USE_DIRECTION_CLASSIFIER': True, 'DIR_OFFSET': 0.78539,
    'DIR_LIMIT_OFFSET': 0.0, 'NUM_DIR_BINS': 2, 'ANCHOR_GENERATOR_CONFIG': ANCHOR_CFG,
    'TARGET_ASSIGNER_CONFIG': {'NAME': 'AxisAlignedTargetAssigner', 'POS_FRACTION': -1.0, 'SAMPLE_SIZE': 512,
                               'NORM_BY_NUM_EXAMPLES': False, 'MATCH_HEIGHT': False, 'BOX_CODER': 'ResidualCoder'},
    'LOSS_CONFIG': {'LOSS_WEIGHTS': {'cls_weight': 1.0, 'loc_weight': 2.0, 'dir_weight': 0.2, 'code_weights': [1.0] * 7}},
}
# golden G25: a feature map of 12 x 10 (H != W) over 9.6 m x 8 m, B = 3, 32 input channels
G25_RANGE = [0.0, -4.0, -3.0, 9.6, 4.0, 1.0]
G25_GRID = [96, 80, 40]                      # voxels; // feature_map_stride 8 -> nx = 12, ny = 10
G25_B, G25_M, G25_CHANNELS, G25_SEED = 3, 9, 32, 2500


# ---- anchors -------------------------------------------------------------------------------------------------------------
def arange32(start, end, step):
    """torch.arange(start, end, step, dtype=float32) on the CPU: the values in float64, then rounded."""
    n = int(math.ceil((end - start) / step))
    return (start + step * np.arange(n, dtype=np.float64)).astype(F)


def generate_anchors(anchor_range, grid_sizes, anchor_cfg=ANCHOR_CFG):
    """-> [(nz, ny, nx, #sizes, #rotations, 7) per anchor class], [anchors per location per class]."""
    r = anchor_range
    out, per_loc = [], []
    for (nx, ny), c in zip(grid_sizes, anchor_cfg):
        sizes, rots, heights = c['anchor_sizes'], c['anchor_rotations'], c['anchor_bottom_heights']
        per_loc.append(len(sizes) * len(rots) * len(heights))
        if c.get('align_center', False):
            xs, ys = (r[3] - r[0]) / nx, (r[4] - r[1]) / ny
            xo, yo = xs / 2, ys / 2
        else:
            xs, ys = (r[3] - r[0]) / (nx - 1), (r[4] - r[1]) / (ny - 1)
            xo, yo = 0, 0
        x, y = arange32(r[0] + xo, r[3] + 1e-5, xs), arange32(r[1] + yo, r[4] + 1e-5, ys)
        z = np.array(heights, F)
        a = np.zeros((len(z), len(y), len(x), len(sizes), len(rots), 7), F)
        a[..., 0] = x[None, None, :, None, None]
        a[..., 1] = y[None, :, None, None, None]
        a[..., 2] = z[:, None, None, None, None]
        a[..., 3:6] = np.array(sizes, F)[None, None, None, :, None, :]
        a[..., 6] = np.array(rots, F)[None, None, None, None, :]
        a[..., 2] = a[..., 2] + a[..., 5] / F(2)
        out.append(a)
    return out, per_loc


def feature_map_sizes(grid, anchor_cfg=ANCHOR_CFG):
    return [(grid[0] // c['feature_map_stride'], grid[1] // c['feature_map_stride']) for c in anchor_cfg]


def flat(all_anchors):
    """The head's flattened order (A, 7): torch.cat(anchors, dim=-3).view(-1, 7)."""
    return np.ascontiguousarray(np.concatenate(all_anchors, axis=-3).reshape(-1, 7))


def class_sets(all_anchors, anchor_cfg=ANCHOR_CFG, class_names=CLASS_NAMES):
    return [(a.shape[3] * a.shape[4], c['matched_threshold'], c['unmatched_threshold'], class_names.index(c['class_name']) + 1)
            for a, c in zip(all_anchors, anchor_cfg)]


# ---- the IoU ---------------------------------------------------------------------------------------------------------------
def limit_period(val):
    return val - np.floor(val / PI + F(0.5)) * PI


def aligned_bev_boxes(boxes):
    boxes = np.asarray(boxes, F)
    rot = np.abs(limit_period(boxes[:, 6]))
    dims = np.where(rot[:, None] < QUARTER, boxes[:, [3, 4]], boxes[:, [4, 3]])
    return np.concatenate((boxes[:, 0:2] - dims / F(2), boxes[:, 0:2] + dims / F(2)), axis=1)


def boxes_iou_normal(a, b):
    x_min = np.maximum(a[:, 0, None], b[None, :, 0])
    x_max = np.minimum(a[:, 2, None], b[None, :, 2])
    y_min = np.maximum(a[:, 1, None], b[None, :, 1])
    y_max = np.minimum(a[:, 3, None], b[None, :, 3])
    x_len = np.maximum(x_max - x_min, F(0))
    y_len = np.maximum(y_max - y_min, F(0))
    area_a = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area_b = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    inter = x_len * y_len
    out = inter / np.maximum(area_a[:, None] + area_b[None, :] - inter, F(1e-6))
    assert out.dtype == F
    return out


def nearest_bev_iou(boxes_a, boxes_b):
    return boxes_iou_normal(aligned_bev_boxes(boxes_a), aligned_bev_boxes(boxes_b))


# ---- the coder -------------------------------------------------------------------------------------------------------------
def encode(boxes, anchors):
    """ResidualCoder.encode_torch (7 columns) on copies, float32; the logarithm is the float64 one, rounded."""
    b, a = np.array(boxes, F), np.array(anchors, F)
    a[:, 3:6] = np.maximum(a[:, 3:6], F(1e-5))
    b[:, 3:6] = np.maximum(b[:, 3:6], F(1e-5))
    diag = np.sqrt(a[:, 3] * a[:, 3] + a[:, 4] * a[:, 4])
    cols = [(b[:, 0] - a[:, 0]) / diag, (b[:, 1] - a[:, 1]) / diag, (b[:, 2] - a[:, 2]) / a[:, 5]]
    cols += [np.log((b[:, k] / a[:, k]).astype(np.float64)).astype(F) for k in (3, 4, 5)]
    cols.append(b[:, 6] - a[:, 6])
    out = np.stack(cols, axis=1)
    assert out.dtype == F
    return out


# ---- the assigner ------------------------------------------------------------------------------------------------------------
def assign_single(anchors, gt_boxes, gt_classes, matched, unmatched, record=None):
    n = anchors.shape[0]
    labels = -np.ones(n, np.int32)
    have = len(gt_boxes) > 0 and n > 0
    if have:
        iou = nearest_bev_iou(anchors[:, 0:7], gt_boxes[:, 0:7])
        arg = iou.argmax(axis=1)                                     # the first of equal maxima
        best = iou[np.arange(n), arg]
        top = iou[iou.argmax(axis=0), np.arange(len(gt_boxes))].copy()
        top[top == 0] = -1
        forced = np.nonzero(iou == top[None, :])[0]
        labels[forced] = gt_classes[arg[forced]]
        pos = best >= F(matched)
        labels[pos] = gt_classes[arg[pos]]
        labels[best < F(unmatched)] = 0
        labels[forced] = gt_classes[arg[forced]]
        if record is not None:
            record.append(dict(iou=iou, arg=arg, best=best, top=top, forced=np.unique(forced), labels=labels.copy()))
    else:
        labels[:] = 0
        if record is not None:
            record.append(None)
    targets = np.zeros((n, 7), F)
    fg = np.nonzero(labels > 0)[0]
    if have and len(fg):
        targets[fg] = encode(gt_boxes[arg[fg], 0:7], anchors[fg])
    weights = np.zeros(n, F)
    weights[labels > 0] = 1.0
    if record is not None and have:
        record[-1]['arg_of_fg'] = np.where(labels > 0, arg, -1)
    return labels, targets, weights


def assign_targets(all_anchors, gt_boxes_with_classes, anchor_cfg=ANCHOR_CFG, class_names=CLASS_NAMES, record=None):
    """all_anchors: [(nz, ny, nx, #size, #rot, 7)]; gt (B, M, 8) -> box_cls_labels int32 (B, A), box_reg_targets (B, A, 7),
    reg_weights (B, A).  record: a list that receives, per (sample, class), the intermediate arrays (None without a box)."""
    gt_all = np.asarray(gt_boxes_with_classes, F)
    names = np.array(class_names)
    out = ([], [], [])
    for k in range(gt_all.shape[0]):
        cur = gt_all[k, :, :-1]
        cnt = len(cur) - 1
        while cnt > 0 and cur[cnt].sum() == 0:
            cnt -= 1
        cur = cur[:cnt + 1]
        classes = gt_all[k, :cnt + 1, -1].astype(np.int32)
        per_class = []
        for c, anchors in zip(anchor_cfg, all_anchors):
            mask = names[classes - 1] == c['class_name'] if len(classes) else np.zeros(0, bool)
            fmap = anchors.shape[:3]
            lab, tgt, wgt = assign_single(anchors.reshape(-1, 7), cur[mask], classes[mask], c['matched_threshold'],
                                          c['unmatched_threshold'], record)
            per_class.append((lab.reshape(*fmap, -1), tgt.reshape(*fmap, -1, 7), wgt.reshape(*fmap, -1)))
        out[0].append(np.concatenate([p[0] for p in per_class], axis=-1).reshape(-1))
        out[1].append(np.concatenate([p[1] for p in per_class], axis=-2).reshape(-1, 7))
        out[2].append(np.concatenate([p[2] for p in per_class], axis=-1).reshape(-1))
    return np.stack(out[0]), np.stack(out[1]), np.stack(out[2])


def foreground_rows(all_anchors, gt_boxes_with_classes, anchor_cfg=ANCHOR_CFG, class_names=CLASS_NAMES):
    """(B, A) int64: for every foreground anchor the ROW of gt_boxes its target is encoded from, -1 elsewhere -- what a
    plain encode_torch on another device needs to evaluate the same targets."""
    gt_all = np.asarray(gt_boxes_with_classes, F)
    rec = []
    labels, _, _ = assign_targets(all_anchors, gt_all, anchor_cfg, class_names, record=rec)
    names = np.array(class_names)
    rows = []
    for k in range(gt_all.shape[0]):
        cnt = len(gt_all[k]) - 1
        while cnt > 0 and gt_all[k, cnt, :-1].sum() == 0:
            cnt -= 1
        classes = gt_all[k, :cnt + 1, -1].astype(np.int32)
        per_class = []
        for j, (c, anchors) in enumerate(zip(anchor_cfg, all_anchors)):
            r = rec[k * len(anchor_cfg) + j]
            own = np.nonzero(names[classes - 1] == c['class_name'])[0] if len(classes) else np.zeros(0, np.int64)
            n = anchors.reshape(-1, 7).shape[0]
            row = np.full(n, -1, np.int64)
            if r is not None:
                fg = r['arg_of_fg'] >= 0
                row[fg] = own[r['arg_of_fg'][fg]]
            per_class.append(row.reshape(*anchors.shape[:3], -1))
        rows.append(np.concatenate(per_class, axis=-1).reshape(-1))
    rows = np.stack(rows)
    assert np.array_equal(rows >= 0, labels > 0)
    return rows


# ---- the cases of the GPU test -------------------------------------------------------------------------------------------------
# x 0 .. 32 and y -8.25 .. 8.25 in steps of 0.5: every node is exact in float32 and the nodes mirror at y = 0, so a box
# on the axis has the same IoU, bit for bit, with the two anchors left and right of it.  65 x 34 locations x 6 anchors =
# 13 260: 51.8 workgroups of 256
CASE_RANGE = [0.0, -8.25, -3.0, 32.0, 8.25, 1.0]
CASE_FMAP = [(65, 34)] * 3
CASE_M = 70


def case_anchors():
    return generate_anchors(CASE_RANGE, CASE_FMAP)[0]


def _rows(rows, M=CASE_M):
    out = np.zeros((M, 8), F)
    if len(rows):
        out[:len(rows)] = np.array(rows, F)
    return out


def car(x, y, h=0.0, z=-1.0, cls=1):
    return [x, y, z, 3.9, 1.6, 1.56, h, cls]


def ped(x, y, h=0.0, z=0.2):
    return [x, y, z, 0.8, 0.6, 1.73, h, 2]


def bike(x, y, h=0.0):
    return [x, y, 0.2, 1.76, 0.6, 1.73, h, 3]


def cases():
    """name -> (M, 8) rows of one sample; every case asserts its own condition with the restatement (check_cases)."""
    rng = np.random.default_rng(77)
    q = math.pi / 4
    out = {}
    out['no_box'] = _rows([])
    out['trailing_zero_rows'] = _rows([car(10.2, 1.1), ped(5.1, -3.0), bike(20.3, 2.2, 1.5)])
    out['interior_zero_row'] = _rows([car(10.2, 1.1), [0] * 8, ped(5.1, -3.0), [0] * 8, [0] * 8, bike(20.3, 2.2, 1.5)])
    out['class_without_box'] = _rows([car(12.0, -2.0, 0.3), ped(7.0, 3.0)])
    out['box_out_of_range'] = _rows([car(100.0, 50.0), ped(6.0, 1.25)])
    # a pedestrian of 5 cm on the mirror axis: nothing reaches matched; the anchors at y = -0.25 and y = +0.25 tie
    out['tiny_box_forced_on_ties'] = _rows([[8.0, 0.0, 0.2, 0.05, 0.05, 1.7, 0.0, 2]])
    # the same footprint twice, different z: the lower row wins every arg max
    out['identical_boxes'] = _rows([ped(9.0, 2.25, z=0.9), ped(9.0, 2.25, z=-0.4), car(15.0, -4.25)])
    # the tiny box forces anchors whose best box is the large one next to it
    out['forced_with_other_argmax'] = _rows([[8.05, 1.25, 0.2, 0.05, 0.05, 1.7, 0.0, 2], [8.0, 1.25, 0.2, 0.9, 0.9, 1.7, 0.0, 2]])
    out['headings_at_quarter_turns'] = _rows([car(4.0 + 3.5 * k, -6.0 + 1.7 * k, s * (m * q + e))
                                              for k, (s, m, e) in enumerate((s, m, e) for s in (1, -1) for m in (1, 3)
                                                                            for e in (-0.01, 0.01))])
    many = []
    for k in range(CASE_M):
        x, y = rng.uniform(1.0, 31.0), rng.uniform(-7.5, 7.5)
        h = rng.uniform(-math.pi, math.pi)
        many.append([car, ped, bike][k % 3](x, y, h))
    out['seventy_boxes'] = _rows(many)
    return out


def check_cases(all_anchors=None):
    """Runs every case through the restatement and asserts the condition it is named after.  -> {name: (labels, targets,
    weights)} of the case as a batch of one."""
    anchors = case_anchors() if all_anchors is None else all_anchors
    cs = cases()
    res, recs = {}, {}
    for name, rows in cs.items():
        rec = []
        res[name] = assign_targets(anchors, rows[None], record=rec)
        recs[name] = rec
    A = res['no_box'][0].shape[1]
    assert A == 65 * 34 * 6 and A % 256 != 0 and A > 8 * 256
    assert not res['no_box'][0].any() and all(r is None for r in recs['no_box'][:2]) and recs['no_box'][2] is not None
    assert recs['no_box'][2]['iou'].shape[1] == 1                                  # the kept zero row, filed under Bicycle
    a, b = res['trailing_zero_rows'], res['interior_zero_row']
    assert (a[0] > 0).sum() > 0 and all(np.array_equal(u, v) for u, v in zip(a, b))
    assert recs['trailing_zero_rows'][2]['iou'].shape[1] == 1 and recs['interior_zero_row'][2]['iou'].shape[1] == 4
    assert recs['class_without_box'][2] is None and set(np.unique(res['class_without_box'][0])) == {-1, 0, 1, 2}
    r = recs['box_out_of_range'][0]
    assert r['top'].tolist() == [-1.0] and len(r['forced']) == 0 and not (res['box_out_of_range'][0] == 1).any()
    r = recs['tiny_box_forced_on_ties'][1]
    assert r['best'].max() < 0.35 and len(r['forced']) >= 2 and (res['tiny_box_forced_on_ties'][0] == 2).sum() == len(r['forced'])
    r = recs['identical_boxes'][1]
    assert np.array_equal(r['iou'][:, 0], r['iou'][:, 1]) and not (r['arg'] == 1).any() and (r['labels'] == 2).any()
    lab, tgt, _ = res['identical_boxes']
    fg = np.nonzero(lab[0] == 2)[0]
    za = flat(anchors)[fg, 2]
    assert np.array_equal(tgt[0, fg, 2], (F(0.9) - za) / F(1.73))
    r = recs['forced_with_other_argmax'][1]
    mine = [a_ for a_ in r['forced'] if r['iou'][a_, 0] == r['top'][0]]
    assert mine and all(r['arg'][a_] == 1 for a_ in mine) and r['top'][0] < 0.35
    rows = cs['headings_at_quarter_turns'][:8]
    rect = aligned_bev_boxes(rows[:, :7])
    wide = (rect[:, 2] - rect[:, 0]) > 2.0
    assert wide.tolist() == [True, False, False, True, True, False, False, True]
    assert len(recs['seventy_boxes'][0]['top']) == 24 and (res['seventy_boxes'][0] > 0).sum() > 70
    assert (cs['seventy_boxes'].sum(1) != 0).all() and CASE_M > 64
    return res


# ---- the model of second_ps.yaml, typed in as plain dicts ----------------------------------------------------------------------
SECOND_MODEL = {
    'NAME': 'SECONDNet',
    'VFE': {'NAME': 'MeanVFE'},
    'BACKBONE_3D': {'NAME': 'VoxelBackBone8x'},
    'MAP_TO_BEV': {'NAME': 'HeightCompression', 'NUM_BEV_FEATURES': 256},
    'BACKBONE_2D': {'NAME': 'BaseBEVBackbone', 'LAYER_NUMS': [5, 5], 'LAYER_STRIDES': [1, 2], 'NUM_FILTERS': [128, 256],
                    'UPSAMPLE_STRIDES': [1, 2], 'NUM_UPSAMPLE_FILTERS': [256, 256]},
    'DENSE_HEAD': HEAD_CFG,
    'POST_PROCESSING': {'RECALL_THRESH_LIST': [0.3, 0.5, 0.7], 'SCORE_THRESH': 0.2, 'OUTPUT_RAW_SCORE': False,
                        'EVAL_METRIC': 'kitti',
                        'NMS_CONFIG': {'MULTI_CLASSES_NMS': False, 'NMS_TYPE': 'nms_gpu', 'NMS_THRESH': 0.01,
                                       'NMS_PRE_MAXSIZE': 4096, 'NMS_POST_MAXSIZE': 500}},
}
