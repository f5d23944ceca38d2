"""NumPy float32 restatement of the reference's anchor target assignment (AxisAlignedTargetAssigner.assign_targets for
POS_FRACTION < 0, NORM_BY_NUM_EXAMPLES False, MATCH_HEIGHT False, no multihead): the loop over samples and anchor
classes, the dense (anchors x boxes) nearest-BEV IoU matrix operation by operation, the two arg maxima, the forced
anchors, the labels, ResidualCoder.encode_torch.  It shares no code with the package's modules.

Also here, because the host test checks them on the CPU with this restatement and the GPU test runs them: the class sets
of cfgs/kitti_models/second_ps.yaml, the anchors of a feature map, the fixture shapes of golden G25 and the CASES of
tests/test_gpu_anchor_target.py, each asserting that the condition it is named after occurs.

For tests/test_gpu_anchor_target_edges.py: assign_flat, the same assignment over class sets given as extents on a flat
block (the C ABI's form: any extents, where the concatenation along the sizes axis needs equal rotation counts), the edge
cases on dyadic coordinates (edge_cases, big_m_cases, batch_limit_case) with their own assertions, and the fixture of golden
G27 (the reference's assigner alone at a layout that is not KITTI's)."""
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


# ---- class sets on a flat block --------------------------------------------------------------------------------------------------
def kept_rows(sample):
    """The reference's cut: trailing rows whose seven values sum to 0 go, row 0 stays."""
    cnt = len(sample) - 1
    while cnt > 0 and sample[cnt, :7].sum() == 0:
        cnt -= 1
    return cnt + 1


def assign_flat_rows(flat_anchors, class_sets, gt, record=None):
    """flat_anchors (A, 7) in the head's order; class_sets [(slots, matched, unmatched, class_id)] -- set s owns the slots
    begin[s] .. begin[s + 1] - 1 of every location, the last set takes class 0 as well; gt (B, M, 8) -> labels int32
    (B, A), targets (B, A, 7), weights (B, A), rows int64 (B, A): the row of gt a foreground target is encoded from, -1
    elsewhere.  Per set: gather its anchors, assign_single, scatter.  record receives per (sample, set) assign_single's
    arrays plus 'idx' (the set's anchors in the block) and 'own' (the set's rows of gt), or None without a box."""
    flat_anchors, gt = np.asarray(flat_anchors, F), np.asarray(gt, F)
    A, (B, M) = flat_anchors.shape[0], gt.shape[:2]
    begin = np.concatenate(([0], np.cumsum([int(s[0]) for s in class_sets])))
    per_loc = int(begin[-1])
    assert A % per_loc == 0
    slot = np.arange(A) % per_loc
    labels, targets = np.zeros((B, A), np.int32), np.zeros((B, A, 7), F)
    weights, rows = np.zeros((B, A), F), np.full((B, A), -1, np.int64)
    for b in range(B):
        n = kept_rows(gt[b]) if M > 0 else 0
        cur = gt[b, :n, :7]
        classes = gt[b, :n, 7].astype(np.int32)
        for s, (_, matched, unmatched, cid) in enumerate(class_sets):
            idx = np.nonzero((slot >= begin[s]) & (slot < begin[s + 1]))[0]
            mask = classes == cid
            if s == len(class_sets) - 1:
                mask = mask | (classes == 0)
            own = np.nonzero(mask)[0]
            rec = [] if record is None else record
            lab, tgt, wgt = assign_single(flat_anchors[idx], cur[own], classes[own], matched, unmatched, rec)
            labels[b, idx], targets[b, idx], weights[b, idx] = lab, tgt, wgt
            if rec[-1] is not None:
                fg = rec[-1]['arg_of_fg'] >= 0
                rows[b, idx[fg]] = own[rec[-1]['arg_of_fg'][fg]]
                rec[-1]['idx'], rec[-1]['own'] = idx, own
    assert np.array_equal(rows >= 0, labels > 0)
    return labels, targets, weights, rows


def assign_flat(flat_anchors, class_sets, gt, record=None):
    return assign_flat_rows(flat_anchors, class_sets, gt, record)[:3]


def foreground_rows_flat(flat_anchors, class_sets, gt):
    return assign_flat_rows(flat_anchors, class_sets, gt)[3]


# ---- the edge cases of the GPU test: dyadic coordinates, every IoU exact in float32 ------------------------------------------------
# slots of a location as (dx, dy, dz, z, heading); locations 2 m apart, so the 2 x 2 anchors of neighbours touch and never
# overlap.  A 1 x 2 box centred in a 2 x 2 anchor: IoU 0.5; 1 x 1 in 2 x 2: 0.25; 0.5 x 0.5 in 1 x 1: 0.25; 1 x 2 in 2 x 1: 1/3
A22, A12, A21, A11 = (2, 2, 2, 0, 0), (1, 2, 2, 0, 0), (2, 1, 2, 0, 0), (1, 1, 1, 0, 0)


def block(nx, ny, slots, step=2.0):
    """(ny * nx * len(slots), 7): locations in y, x order at (step * i, step * j), the slots one after another."""
    out = np.zeros((ny, nx, len(slots), 7), F)
    out[..., 0] = (step * np.arange(nx))[None, :, None]
    out[..., 1] = (step * np.arange(ny))[:, None, None]
    for k, (dx, dy, dz, z, h) in enumerate(slots):
        out[:, :, k, 2:7] = [z, dx, dy, dz, h]
    return np.ascontiguousarray(out.reshape(-1, 7))


# name -> (slots, class sets).  's8': a permutation of 1 .. 8 with the largest last; 'uneven': classes 2 and 4 have no set;
# 'g27': the extents of golden G27.  Set 1 of 'uneven', set 5 of 's8' and set 0 of 'g27' have unmatched == matched
LAYOUTS = {
    's1': ([A22, A12], [(2, 0.5, 0.25, 1)]),
    's8': ([A22, A12, A11, A21, A22, A12, A11, A22],
           [(1, 0.5, 0.25, 3), (1, 0.75, 0.5, 1), (1, 0.5, 0.25, 4), (1, 0.75, 0.25, 2), (1, 0.5, 0.25, 7), (1, 0.5, 0.5, 5),
            (1, 0.75, 0.5, 6), (1, 0.5, 0.25, 8)]),
    'uneven': ([A22, A22, A12, A11, A21, A22, A12, A11], [(1, 0.5, 0.25, 3), (4, 0.5, 0.5, 1), (3, 0.75, 0.25, 5)]),
    'g27': ([A22, A22, A22, A22, A12, A21, A11, A12, A21, A11, A11, A11],
            [(3, 0.5, 0.5, 3), (6, 0.5, 0.25, 1), (3, 0.75, 0.25, 5)]),
    'kitti6': ([A22, A12, A22, A21, A11, A11], [(2, 0.5, 0.25, 1), (2, 0.5, 0.5, 2), (2, 0.75, 0.25, 3)]),
}
EDGE_NAMES = ['s1_on_matched', 's1_on_unmatched', 's8_every_class', 'equal_thresholds', 'class_without_set', 'class0_real_box',
              'flat_boxes', 'clamped_anchor', 'zero_extent', 'negative_extent', 'exact_headings', 'cancelling_trailing_row',
              'g27_layout', 'a6_b1', 'a252', 'a768', 'a1536', 'b300_a768']
BIG_M_NAMES = ['m512_all_live', 'm512_live_from_300', 'm257_row_256']
EDGE_NX, EDGE_NY = 9, 7                      # 63 locations: with 8 slots 504 anchors, two workgroups, the second part full


def gbox(x, y, dx, dy, cls, h=0.0, z=0.0, dz=2.0):
    return [x, y, z, dx, dy, dz, h, cls]


def scatter_boxes(seed, n, classes, nx=EDGE_NX, ny=EDGE_NY, off=()):
    """n boxes on quarter-metre coordinates with dyadic extents and headings near 0 or a quarter turn, none of them over an
    anchor at one of the centres `off` (extents up to 2.5 m: 2.5 m away in x or in y)."""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        k = len(out)
        x, y = rng.integers(0, 8 * (nx - 1) + 1) / 4.0, rng.integers(0, 8 * (ny - 1) + 1) / 4.0
        if any(abs(x - u) < 2.5 and abs(y - v) < 2.5 for u, v in off):
            continue
        out.append(gbox(x, y,
                        [0.5, 1.0, 1.5, 2.0, 2.5][rng.integers(5)], [0.5, 1.0, 1.5, 2.0, 2.5][rng.integers(5)],
                        classes[k % len(classes)], [0.0, 1.5, -0.25, 3.0][rng.integers(4)], rng.integers(-4, 5) / 4.0,
                        [1.0, 2.0, 1.5][rng.integers(3)]))
    return out


def _case(layout, rows, M=None, nx=EDGE_NX, ny=EDGE_NY, flat_block=None):
    slots, sets = LAYOUTS[layout]
    gt = np.zeros((1, M if M is not None else len(rows) + 2, 8), F)            # two trailing zero rows by default
    if len(rows):
        gt[0, :len(rows)] = np.array(rows, F)
    return dict(flat=block(nx, ny, slots) if flat_block is None else flat_block, sets=sets, gt=gt)


def _without_rows(gt, drop):
    keep = [k for k in range(gt.shape[1]) if k not in drop]
    out = np.zeros_like(gt)
    out[0, :len(keep)] = gt[0, keep]
    return out


def _set_of(rec, sets, s, b=0):
    return rec[b * len(sets) + s]


def edge_cases():
    """name -> dict(flat (A, 7), sets, gt (B, M, 8)).  check_edge_cases asserts for each the condition it is named after."""
    q = QUARTER
    out = {}
    # S = 1.  The 1 x 2 box: slot A12 has IoU 1 (top, forced), slot A22 exactly 0.5 = matched and is not forced.
    out['s1_on_matched'] = _case('s1', [gbox(4, 4, 1, 2, 1)] + scatter_boxes(1, 6, [1], off=[(4, 4)]))
    # the 1 x 1 box: A12 has 0.5 (top), A22 exactly 0.25 = unmatched: -1, not 0
    out['s1_on_unmatched'] = _case('s1', [gbox(8, 6, 1, 1, 1)] + scatter_boxes(2, 6, [1], off=[(8, 6)]))
    # S = 8, one slot each, every class 0 .. 8 present, thresholds differing from set to set
    # the box at x = 12.875: IoU 0.391 with the anchor at 12 (top, forced), 0.28 with the one at 14: between the thresholds
    out['s8_every_class'] = _case('s8', [gbox(2 * c, 2 * (c % 5 + 1), 1, 2, c) for c in range(9)] + [gbox(12.875, 2, 2, 2, 3)]
                                  + scatter_boxes(3, 26, list(range(9))))
    # set 1 of 'uneven' (slots 1 .. 4, class 1) has unmatched == matched == 0.5
    out['equal_thresholds'] = _case('uneven', [gbox(6, 4, 1, 2, 1)] + scatter_boxes(4, 12, [1, 3, 5], off=[(6, 4)]))
    # rows 1, 3 and 6 are of the classes 2 and 4, which no set takes
    rows = scatter_boxes(5, 8, [3, 1, 5], off=[(4, 4)])
    rows[1][7], rows[3][7], rows[6][7] = 2, 4, 2
    rows[1][:2], rows[1][3:5] = [4, 4], [2, 2]                                        # a footprint that would be a perfect match
    out['class_without_set'] = _case('uneven', rows)
    # row 0: class 0, alone at (12, 8), equal to slot A22 of the last set: forces it, label 0.  Rows 1, 2 at (4, 6): the
    # class-5 box 1 x 2 has IoU 0.5 with A22, the class-0 box 2 x 2 has IoU 1: it wins the arg max, label 0 instead of -1
    out['class0_real_box'] = _case('uneven', [gbox(12, 8, 2, 2, 0), gbox(4, 6, 1, 2, 5), gbox(4, 6, 2, 2, 0)]
                                   + scatter_boxes(6, 6, [3, 1, 5, 0], off=[(12, 8), (4, 6)]))
    # dz == 0 and dz < 0 on boxes that are a perfect match of an anchor
    out['flat_boxes'] = _case('s1', [gbox(4, 4, 2, 2, 1, dz=0.0), gbox(10, 8, 1, 2, 1, dz=-1.5)])
    blk = block(EDGE_NX, EDGE_NY, LAYOUTS['s1'][0])
    at = (2 * EDGE_NX + 3) * 2                                                         # slot A22 at (6, 4)
    assert blk[at, :2].tolist() == [6, 4]
    blk[at, 5] = 0.0
    out['clamped_anchor'] = _case('s1', [gbox(6, 4, 2, 2, 1, z=0.5)], flat_block=blk)
    out['zero_extent'] = _case('s1', [gbox(4, 4, 0, 2, 1), gbox(8, 8, 1, 2, 1)])
    out['negative_extent'] = _case('s1', [gbox(4, 4, -2, 2, 1), gbox(8, 8, 1, 2, 1), gbox(12, 4, -1, -2, 1)])
    hs = [s * v for v in (q, PI, F(100.0), F(3) * q) for s in (F(1), F(-1))]
    out['exact_headings'] = _case('uneven', [gbox(2 + 2 * k, 2 + 2 * (k % 4), 1, 2, 1, h=float(h)) for k, h in enumerate(hs)])
    # the last row: 4 + 4 - 12 + 2 + 2 + 0 + 0 = 0 with a footprint equal to an anchor's: cut, as in the reference
    out['cancelling_trailing_row'] = _case('s1', [gbox(8, 8, 1, 2, 1), gbox(4, 4, 2, 2, 1, z=-12.0, dz=0.0)], M=2)
    out['g27_layout'] = _case('g27', [gbox(4, 4, 1, 2, 3), gbox(8, 6, 1, 2, 1), gbox(12, 8, 1, 1, 1), gbox(6, 10, 0.5, 0.5, 5)]
                              + scatter_boxes(7, 16, [3, 1, 5, 0, 2, 4], off=[(4, 4), (8, 6), (12, 8), (6, 10)]))
    # ---- shapes: A below a workgroup, one location, multiples of 256; B in the hundreds and at the limit
    out['a6_b1'] = _case('kitti6', [gbox(0, 0, 1, 2, 1), gbox(0, 0, 1, 1, 3), gbox(0, 0, 1, 1, 2)], nx=1, ny=1)
    out['a252'] = _case('kitti6', scatter_boxes(8, 9, [1, 2, 3, 0], 7, 6), nx=7, ny=6)
    out['a768'] = _case('kitti6', scatter_boxes(9, 12, [1, 2, 3, 0], 16, 8), nx=16, ny=8)
    out['a1536'] = _case('kitti6', scatter_boxes(10, 12, [1, 2, 3, 0], 16, 16), nx=16, ny=16)
    many = np.zeros((300, 5, 8), F)
    for b in range(300):
        many[b, :b % 6] = np.array(scatter_boxes(1000 + b, 5, [1, 2, 3, 0], 16, 8), F)[:b % 6]
    out['b300_a768'] = dict(flat=block(16, 8, LAYOUTS['kitti6'][0]), sets=LAYOUTS['kitti6'][1], gt=many)
    return out


def check_edge_cases():
    """-> {name: (case, (labels, targets, weights, rows))}, every condition asserted with the restatement."""
    cs = edge_cases()
    res, recs = {}, {}
    for name, c in cs.items():
        rec = []
        res[name] = (c, assign_flat_rows(c['flat'], c['sets'], c['gt'], rec))
        recs[name] = rec
    lab = {name: r[1][0][0] for name, r in res.items()}

    def loose(r):                                       # anchors of the set (positions in it) that no box forces
        return np.setdiff1d(np.arange(len(r['best'])), r['forced'])

    r = recs['s1_on_matched'][0]
    on = [a for a in loose(r) if r['best'][a] == F(0.5)]
    assert on and all(r['labels'][a] == 1 for a in on) and LAYOUTS['s1'][1][0][1] == 0.5
    assert cs['s1_on_matched']['flat'].shape[0] == 126                        # below one workgroup
    r = recs['s1_on_unmatched'][0]
    on = [a for a in loose(r) if r['best'][a] == F(0.25)]
    assert on and all(r['labels'][a] == -1 for a in on) and LAYOUTS['s1'][1][0][2] == 0.25
    assert all(r['iou'][:, r['arg'][a]].max() > F(0.25) for a in on)
    rec = recs['s8_every_class']
    assert len(rec) == 8 and all(x is not None for x in rec) and sorted(s[3] for s in LAYOUTS['s8'][1]) == list(range(1, 9))
    assert [x['iou'].shape[1] for x in rec] == [5] + [4] * 6 + [7] and LAYOUTS['s8'][1][-1][3] == 8
    assert set(np.unique(lab['s8_every_class'])) == set(range(-1, 9)) and cs['s8_every_class']['flat'].shape[0] == 504
    assert all((x['labels'] > 0).any() for x in rec)
    r = recs['equal_thresholds'][1]
    on = [a for a in loose(r) if r['best'][a] == F(0.5)]
    assert LAYOUTS['uneven'][1][1][1:3] == (0.5, 0.5) and not (r['labels'] == -1).any() and on
    assert all(r['labels'][a] == 1 for a in on) and ((r['best'] > 0) & (r['best'] < F(0.5))).any()
    assert (recs['equal_thresholds'][0]['labels'] == -1).any() or (recs['equal_thresholds'][2]['labels'] == -1).any()
    c = cs['class_without_set']
    assert c['gt'][0, [1, 3, 6], 7].tolist() == [2, 4, 2]
    without = assign_flat(c['flat'], c['sets'], _without_rows(c['gt'], (1, 3, 6)))
    assert all(u.tobytes() == v.tobytes() for u, v in zip(res['class_without_set'][1][:3], without))
    assert (lab['class_without_set'] > 0).any() and not (c['flat'][lab['class_without_set'] > 0, :2] == [4, 4]).all(1).any()
    c, r = cs['class0_real_box'], recs['class0_real_box'][2]
    col = list(r['own']).index(0)
    mine = [a for a in r['forced'] if r['iou'][a, col] == r['top'][col]]
    assert r['top'][col] == 1 and mine and all(r['arg'][a] == col and r['labels'][a] == 0 for a in mine)
    assert not res['class0_real_box'][1][2][0, r['idx'][mine]].any()
    win = [a for a in range(len(r['best'])) if r['arg'][a] == list(r['own']).index(2) and r['iou'][a, list(r['own']).index(1)] == F(0.5)]
    assert win and all(r['labels'][a] == 0 for a in win)
    alone = assign_flat(c['flat'], c['sets'], _without_rows(c['gt'], (0, 2)))
    assert all(alone[0][0, r['idx'][a]] == -1 for a in win)
    c, (_, tgt, _, rows) = res['flat_boxes']
    for k, za in ((0, 2.0), (1, 2.0)):
        fg = np.nonzero(rows[0] == k)[0]
        assert len(fg) and np.array_equal(tgt[0, fg, 5], np.full(len(fg), np.log(np.float64(F(1e-5) / F(za))), F))
    c, (_, tgt, _, rows) = res['clamped_anchor']
    at = np.nonzero(c['flat'][:, 5] == 0)[0]
    assert len(at) == 1 and rows[0, at[0]] == 0 and tgt[0, at[0], 2] == F(0.5) / F(1e-5)
    assert tgt[0, at[0], 5] == F(np.log(np.float64(F(2.0) / F(1e-5))))
    r = recs['zero_extent'][0]
    assert r['top'][0] == -1 and not (r['iou'][:, 0] > 0).any() and (r['labels'] == 1).sum() == 2
    r = recs['negative_extent'][0]
    a, b = aligned_bev_boxes(cs['negative_extent']['flat']), aligned_bev_boxes(cs['negative_extent']['gt'][0, :3, :7])
    uni = ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] + ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :]
    assert (uni[:, 0] < F(1e-6)).any() and r['top'].tolist() == [-1, 1, -1] and (r['labels'] == 1).sum() == 2
    c = cs['exact_headings']
    rect = aligned_bev_boxes(c['gt'][0, :8, :7])
    assert c['gt'][0, :8, 6].tolist() == [QUARTER, -QUARTER, PI, -PI, 100.0, -100.0, F(3) * QUARTER, -F(3) * QUARTER]
    assert ((rect[:, 2] - rect[:, 0]) > 1.5).tolist() == [True, True, False, False, False, False, True, True]
    rows = res['exact_headings'][1][3][0]           # slots 1 (A22) and 3 (A11): 0.5 = matched; 2 is A12, 4 is A21 (the swap)
    assert [sorted((np.nonzero(rows == k)[0] % 8).tolist()) for k in range(8)] == [[1, 3, 4]] * 2 + [[1, 2, 3]] * 4 + [[1, 3, 4]] * 2
    c = cs['cancelling_trailing_row']
    assert c['gt'][0, 1, :7].any() and c['gt'][0, 1, :7].sum() == 0 and kept_rows(c['gt'][0]) == 1
    assert recs['cancelling_trailing_row'][0]['iou'].shape[1] == 1 and (lab['cancelling_trailing_row'] == 1).sum() == 2
    assert (assign_flat(c['flat'], c['sets'], c['gt'][:, ::-1].copy())[0] == 1).sum() > 2         # kept when it is not last
    rec = recs['g27_layout']
    assert [len(x['idx']) for x in rec] == [63 * 3, 63 * 6, 63 * 3] and set(np.unique(lab['g27_layout'])) == {-1, 0, 1, 3, 5}
    assert not (rec[0]['labels'] == -1).any() and (rec[1]['labels'] == -1).any()
    for name, A, B in (('a6_b1', 6, 1), ('a252', 252, 1), ('a768', 768, 1), ('a1536', 1536, 1), ('b300_a768', 768, 300)):
        assert res[name][1][0].shape == (B, A) and (res[name][1][0] > 0).any(), name
    assert set(np.unique(lab['a6_b1'])) == {0, 1, 2, 3}
    return res


def batch_limit_case(B=65535):
    """B at DFU3D_ANC_MAX_BATCH, A = 6, M = 1: seven distinct samples in turn -> (case, (labels, targets, weights, rows))
    with the restatement run once per distinct sample."""
    slots, sets = LAYOUTS['kitti6']
    one = np.array([[0] * 8, gbox(0, 0, 1, 2, 1), gbox(0, 0, 2, 2, 2), gbox(0, 0, 1, 1, 3), gbox(0, 0, 2, 2, 0), gbox(0, 0, 2, 1, 1),
                    gbox(0.5, 0, 1, 1, 3, z=0.5)], F)[:, None, :]
    flat_block = block(1, 1, slots)
    want = assign_flat_rows(flat_block, sets, one)
    pick = (np.arange(B) + 1) % len(one)                  # the first and the last sample hold a box
    assert all((want[0][k] > 0).any() for k in (1, 2, 3, 5, 6)) and not want[0][0].any() and not (want[0][4] > 0).any()
    return dict(flat=flat_block, sets=sets, gt=np.ascontiguousarray(one[pick])), tuple(np.ascontiguousarray(w[pick]) for w in want)


# ---- M up to 512 on the 13 260-anchor grid of the cases, the three KITTI sets -------------------------------------------------------
def big_m_cases():
    rng = np.random.default_rng(512)
    rows = []
    for k in range(512):
        rows.append([car, ped, bike][k % 3](rng.uniform(1.0, 31.0), rng.uniform(-7.5, 7.5), rng.uniform(-math.pi, math.pi)))
    full = _rows(rows, 512)
    late = full.copy()
    late[:300] = 0
    one = np.zeros((257, 8), F)
    one[256] = car(10.2, 1.1)
    return {'m512_all_live': full, 'm512_live_from_300': late, 'm257_row_256': one}


def check_big_m_cases(all_anchors=None):
    """-> {name: (gt (1, M, 8), (labels, targets, weights, rows))} with flat anchors and sets of the KITTI case layout."""
    anchors = case_anchors() if all_anchors is None else all_anchors
    fl, sets = flat(anchors), class_sets(anchors)
    res = {}
    for name, rows in big_m_cases().items():
        rec = []
        out = assign_flat_rows(fl, sets, rows[None], rec)
        res[name] = (rows[None], out)
        used = out[3][out[3] >= 0]
        base = np.cumsum([0] + [0 if r is None else r['iou'].shape[1] for r in rec])       # the stage's list: set after set
        forced_at = [base[s] + g for s, r in enumerate(rec) if r is not None
                     for g in np.nonzero((r['iou'] == r['top'][None, :]).any(0))[0]]
        if name == 'm512_all_live':
            assert (rows[:, :7].sum(1) != 0).all() and (used >= 256).any() and (used >= 448).any() and (used < 64).any()
            assert max(forced_at) >= 256 and (out[0] > 0).sum() > 512 and [r['iou'].shape[1] for r in rec] == [171, 171, 170]
        elif name == 'm512_live_from_300':
            assert used.min() >= 300 and (used >= 448).any() and rec[2]['iou'].shape[1] == 300 + 70 and max(forced_at) >= 256
            assert not rows[:300].any() and base[2] < 256 < base[3]
        else:
            assert set(used.tolist()) == {256} and rec[0]['iou'].shape[1] == 1 and rec[2]['iou'].shape[1] == 256 and rec[1] is None
            assert forced_at == [0] and (out[0] == 1).sum() >= 1
    return res


# ---- golden G27: the reference's assigner alone, five class names, sets of 3, 6 and 3 slots ------------------------------------
G27_CLASS_NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Van', 'Truck']
G27_RANGE = [0.0, -16.0, -3.0, 32.0, 16.0, 1.0]
G27_GRID = [136, 136, 40]                    # // feature_map_stride 8 -> 17 x 17 locations 2 m apart
G27_ROTATIONS = [0, 1.57, 3.0]
G27_ANCHOR_CFG = [
    {'class_name': 'Cyclist', 'anchor_sizes': [[2.0, 2.0, 2.0]], 'anchor_rotations': G27_ROTATIONS, 'anchor_bottom_heights': [-1.0],
     'align_center': False, 'feature_map_stride': 8, 'matched_threshold': 0.5, 'unmatched_threshold': 0.5},
    {'class_name': 'Car', 'anchor_sizes': [[2.0, 2.0, 2.0], [1.0, 2.0, 2.0]], 'anchor_rotations': G27_ROTATIONS,
     'anchor_bottom_heights': [-1.0], 'align_center': False, 'feature_map_stride': 8, 'matched_threshold': 0.5,
     'unmatched_threshold': 0.25},
    {'class_name': 'Truck', 'anchor_sizes': [[1.0, 1.0, 1.0]], 'anchor_rotations': G27_ROTATIONS, 'anchor_bottom_heights': [-0.5],
     'align_center': False, 'feature_map_stride': 8, 'matched_threshold': 0.75, 'unmatched_threshold': 0.25},
]
G27_HEAD_CFG = dict(HEAD_CFG, ANCHOR_GENERATOR_CONFIG=G27_ANCHOR_CFG)
G27_B, G27_M, G27_SEED = 3, 14, 2700


def g27_boxes():
    """(3, 14, 8).  Sample 0: boxes on the thresholds of the Car set (0.5 = matched, 0.25 = unmatched) and of the Cyclist set
    (unmatched == matched == 0.5).  Sample 1: rows of the classes 2 and 4 that no set takes, and class-0 rows with a real
    footprint: one alone, one that wins the arg max over a Truck.  Sample 2: boxes off the grid, trailing zero rows."""
    rng = np.random.default_rng(G27_SEED)

    def b(x, y, dx, dy, cls, h=0.0, z=0.0, dz=2.0):
        return [x, y - 16.0, z, dx, dy, dz, h, cls]

    def loose(n, classes):
        out = []
        for k in range(n):
            out.append(b(rng.integers(8, 120) / 4.0, rng.integers(8, 120) / 4.0, [0.5, 1.0, 1.5, 2.0, 2.5][rng.integers(5)],
                         [0.5, 1.0, 1.5, 2.0, 2.5][rng.integers(5)], classes[k % len(classes)],
                         [0.0, 1.5, -0.25, 3.0, float(QUARTER)][rng.integers(5)], rng.integers(-4, 5) / 4.0))
        return out
    gt = np.zeros((G27_B, G27_M, 8), F)
    s0 = [b(4, 4, 1, 2, 1), b(10, 6, 1, 1, 1), b(20, 10, 1, 2, 3), b(26, 24, 0.5, 0.5, 5)] + loose(8, [1, 3, 5])
    s1 = [b(6, 6, 2, 2, 2), b(12, 20, 1, 1, 0), [0] * 8, b(20, 8, 0.5, 1, 5), b(20, 8, 1, 1, 0), b(8, 24, 1, 2, 4)] \
        + loose(8, [1, 2, 3, 4, 5, 0])
    s2 = loose(9, [5, 1, 3])
    for k, rows in enumerate((s0, s1, s2)):
        gt[k, :len(rows)] = np.array(rows, F)
    return gt


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
