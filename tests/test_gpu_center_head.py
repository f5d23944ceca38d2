"""GPU: row f-6, `assign_targets` / `decode_bbox_from_heatmap` / `generate_predicted_boxes` of dfu3d_amd.pcdet_kitti on
csrc/centerhead_stage.hip, against golden G12 (the reference's own run) and the NumPy restatement
(tests/center_head_ref.py).  Bit-equal: cells, inds, masks, target_boxes_src, target_boxes[:, 0:3] and the velocity
columns, and of the decode the order, labels, scores, xs, ys and every gathered column.  Heat maps: the same support and at
most 1 float32 ulp per cell (the device's fp64 exp is within 1 ulp of fp64 and is rounded to float32 once more; the reference
rounds the fp64 value once).  log / cos / sin / atan2 columns: within 1 float32 ulp (see tests/test_oracle_center_head.py)."""
import numpy as np
import pytest

from tests import center_head_ref as ref
from tests.test_oracle_center_head import CFGS, check_assign, check_decode, decode_case_inputs, g12, meta_of  # noqa: F401

pytestmark = pytest.mark.gpu

POST = dict(SCORE_THRESH=0.1, POST_CENTER_LIMIT_RANGE=[0, -61.2, -10.0, 61.2, 61.2, 10.0], MAX_OBJ_PER_SAMPLE=500,
            NMS_CONFIG=dict(MULTI_CLASSES_NMS=True, NMS_TYPE='nms_gpu', NMS_THRESH=0.6, NMS_PRE_MAXSIZE=1000,
                            NMS_POST_MAXSIZE=83))


def make_head(cfg, **over):
    from dfu3d_amd.pcdet_kitti.center_head import CenterHead
    c = dict(cfg, **over)
    model_cfg = dict(CLASS_NAMES_EACH_HEAD=c['heads'], POST_PROCESSING=POST,
                     SEPARATE_HEAD_CFG=dict(HEAD_ORDER=['center', 'center_z', 'dim', 'rot'] + (['vel'] if c['C'] == 10 else [])),
                     TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=c['stride'], NUM_MAX_OBJS=c['num_max_objs'],
                                                 GAUSSIAN_OVERLAP=c['gaussian_overlap'], MIN_RADIUS=c['min_radius']))
    return CenterHead(model_cfg, c['class_names'], np.array(c['point_cloud_range'], np.float32), c['voxel_size'])


def to_np(ret):
    return {k: [t.cpu().numpy() for t in v] for k, v in ret.items()}


def compare_assign(got, want, label):
    """`got` from the GPU, `want` from the restatement (dicts of NumPy arrays per head) under the rules of the module."""
    same = cells = 0
    for h in range(len(want['inds'])):
        assert np.array_equal(got['inds'][h], want['inds'][h]), (label, h)
        assert np.array_equal(got['masks'][h], want['masks'][h]), (label, h)
        assert got['target_boxes_src'][h].tobytes() == want['target_boxes_src'][h].tobytes(), (label, h)
        tb, wb = got['target_boxes'][h], want['target_boxes'][h]
        assert tb[..., 0:3].tobytes() == wb[..., 0:3].tobytes() and tb[..., 8:].tobytes() == wb[..., 8:].tobytes(), (label, h)
        assert ref.ulp_diff(tb[..., 3:8], wb[..., 3:8]).max(initial=0) <= 1, (label, h)
        hm, wm = got['heatmaps'][h], want['heatmaps'][h]
        assert hm.shape == wm.shape and np.array_equal(hm != 0, wm != 0), (label, h)
        assert ref.ulp_diff(hm, wm).max(initial=0) <= 1, (label, h)
        same += int((hm.view(np.uint32) == wm.view(np.uint32)).sum())
        cells += hm.size
    return same, cells


def random_boxes(rng, cfg, B, M, n_max, n_exact=None):
    r = cfg['point_cloud_range']
    C, n_cls = cfg['C'], len(cfg['class_names'])
    gt = np.zeros((B, M, C), np.float32)
    for b in range(B):
        n = int(rng.integers(0, n_max + 1)) if n_exact is None else n_exact
        rows = np.sort(rng.choice(M, n, replace=False))
        g = np.zeros((n, C), np.float32)
        g[:, 0] = rng.uniform(r[0] - 4, r[3] + 4, n)
        g[:, 1] = rng.uniform(r[1] - 4, r[4] + 4, n)
        g[:, 2] = rng.uniform(-5, 3, n)
        g[:, 3] = rng.uniform(0.3, 12, n)
        g[:, 4] = rng.uniform(0.3, 4, n)
        g[:, 5] = rng.uniform(0.5, 4, n)
        g[:, 6] = rng.uniform(-4, 4, n)
        g[:, 7:C - 1] = rng.uniform(-8, 8, (n, C - 8))
        g[:, -1] = rng.integers(1, n_cls + 1, n)
        g[rng.random(n) < 0.02, 3] = 0.0
        gt[b, rows] = g
    return gt


@pytest.mark.parametrize("name", ["A", "B"])
def test_assign_matches_reference_golden(g12, name):
    import torch
    cfg = CFGS[name]
    head = make_head(cfg)
    gt_np = g12[name + "_gt_boxes"]
    gt = torch.from_numpy(gt_np.copy()).cuda()
    ret = head.assign_targets(gt, feature_map_size=list(cfg['map_hw']), check=True)
    assert ret['heatmap_masks'] == []
    assert all(t.is_contiguous() for k in ('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src') for t in ret[k])
    assert np.array_equal(gt.cpu().numpy(), gt_np), "assign_targets wrote into the caller's gt_boxes"
    got = to_np(ret)
    same, cells = check_assign(got, g12, name, exact_heat=False)
    nz = sum(int((h != 0).sum()) for h in got['heatmaps'])
    print("G12 %s: %d of %d heat-map cells bit-equal (%d non-zero)" % (name, same, cells, nz))
    again = to_np(head.assign_targets(gt, feature_map_size=list(cfg['map_hw']), check=True))
    for k in ('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src'):
        for a, b in zip(got[k], again[k]):
            assert a.tobytes() == b.tobytes(), k


@pytest.mark.parametrize("name", ["A", "B"])
def test_assign_overflow_sets_status_and_raises(g12, name):
    import torch
    from dfu3d_amd import stages
    from dfu3d_amd._lib import Dfu3dError
    cfg = CFGS[name]
    head = make_head(cfg)
    over = torch.from_numpy(g12[name + "_over_gt_boxes"]).cuda()
    with pytest.raises(Dfu3dError, match="NUM_MAX_OBJS"):
        head.assign_targets(over, feature_map_size=list(cfg['map_hw']), check=True)
    ret = head.assign_targets(over, feature_map_size=list(cfg['map_hw']))          # no check: the status is exposed
    assert int(head.status.item()) & stages.ST_CENTER_OVERFLOW
    assert int(ret['masks'][0].sum()) == cfg['num_max_objs']                       # only the first NUM_MAX_OBJS slots
    want = ref.assign_targets(g12[name + "_over_gt_boxes"][:, :cfg['num_max_objs']], cfg)
    assert ret['target_boxes_src'][0].cpu().numpy().tobytes() == want['target_boxes_src'][0].tobytes()
    head.assign_targets(over[:, :cfg['num_max_objs']].contiguous(), feature_map_size=list(cfg['map_hw']), check=True)
    assert int(head.status.item()) == 0


def test_assign_random_batches_match_restatement():
    import torch
    rng = np.random.default_rng(61)
    cfg = CFGS["A"]
    gt = random_boxes(rng, cfg, 32, 512, 500)
    gt[1] = random_boxes(rng, dict(cfg, class_names=['Car']), 1, 512, 500, n_exact=500)[0]   # a full head: 500 cars
    head = make_head(cfg)
    got = to_np(head.assign_targets(torch.from_numpy(gt).cuda(), feature_map_size=list(cfg['map_hw']), check=True))
    same, cells = compare_assign(got, ref.assign_targets(gt, cfg), "A, B = 32")
    print("random A: %d of %d heat-map cells bit-equal" % (same, cells))
    # a 180 x 180 map with stride 8
    cfg2 = dict(cfg, point_cloud_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], voxel_size=[0.075, 0.075, 0.2], stride=8,
                map_hw=(180, 180), C=10)
    gt2 = random_boxes(rng, cfg2, 4, 300, 200)
    got2 = to_np(make_head(cfg2).assign_targets(torch.from_numpy(gt2).cuda(), feature_map_size=[180, 180], check=True))
    compare_assign(got2, ref.assign_targets(gt2, cfg2), "180 x 180")


def test_assign_empty_batches():
    import torch
    cfg = CFGS["A"]
    head = make_head(cfg)
    H, W = cfg['map_hw']
    ret = head.assign_targets(torch.zeros((2, 0, 8), device='cuda'), feature_map_size=[H, W], check=True)
    assert [tuple(t.shape) for t in ret['heatmaps']] == [(2, len(h), H, W) for h in cfg['heads']]
    for k in ('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src'):
        assert all(not bool(t.any()) for t in ret[k]), k
    assert ret['target_boxes'][0].shape == (2, 500, 8) and ret['inds'][0].dtype == torch.int64
    ret = head.assign_targets(torch.zeros((0, 5, 8), device='cuda'), feature_map_size=[H, W], check=True)
    assert [tuple(t.shape) for t in ret['heatmaps']] == [(0, len(h), H, W) for h in cfg['heads']]
    assert ret['target_boxes'][0].shape == (0, 500, 8)


def test_assign_makes_no_device_to_host_copy(g12):
    """No synchronisation and no device-to-host copy in assign_targets (check=False): torch's sync debug mode raises on
    any synchronising call of torch's own; the library itself never synchronises (include/dfu3d.h)."""
    import torch
    cfg = CFGS["A"]
    head = make_head(cfg)
    gt = torch.from_numpy(g12["A_gt_boxes"].copy()).cuda()
    head.assign_targets(gt, feature_map_size=list(cfg['map_hw']))                  # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        ret = head.assign_targets(gt, feature_map_size=list(cfg['map_hw']))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(ret['masks'][0].sum()) > 0


def run_decode(d, case_K, thresh, limit, cfg=ref.CFG_A):
    import torch
    from dfu3d_amd.pcdet_kitti import centernet_utils
    t = {k: (None if v is None else torch.from_numpy(v).cuda()) for k, v in d.items()}
    res = centernet_utils.decode_bbox_from_heatmap(
        heatmap=t['heatmap'], rot_cos=t['rot_cos'], rot_sin=t['rot_sin'], center=t['center'], center_z=t['center_z'],
        dim=t['dim'], vel=t['vel'], iou=t['iou'], point_cloud_range=np.array(cfg['point_cloud_range'], np.float32),
        voxel_size=cfg['voxel_size'], feature_map_stride=cfg['stride'], K=case_K, score_thresh=thresh,
        post_center_limit_range=torch.tensor(limit).float().cuda())
    return [{k: v.cpu().numpy() for k, v in r.items()} for r in res]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_decode_matches_reference_golden(g12, i):
    case, d = decode_case_inputs(g12, i)
    limit = meta_of(g12)["decode_limit"]
    got = run_decode(d, case["K"], case["score_thresh"], limit)
    for b, r in enumerate(got):
        check_decode(r, g12, i, b)
    again = run_decode(d, case["K"], case["score_thresh"], limit)
    for a, b in zip(got, again):
        assert all(a[k].tobytes() == b[k].tobytes() for k in a)


def compare_decode(got, want):
    for g, w in zip(got, want):
        assert np.array_equal(g['pred_labels'], w['pred_labels'])
        assert g['pred_scores'].tobytes() == w['pred_scores'].tobytes()
        cols = [c for c in range(w['pred_boxes'].shape[1]) if c != 6]
        assert g['pred_boxes'].shape == w['pred_boxes'].shape
        assert g['pred_boxes'][:, cols].tobytes() == w['pred_boxes'][:, cols].tobytes()
        assert ref.ulp_diff(g['pred_boxes'][:, 6], w['pred_boxes'][:, 6]).max(initial=0) <= 1
        if 'pred_iou' in w:
            assert g['pred_iou'].tobytes() == w['pred_iou'].tobytes()


def test_decode_random_large_map_and_empty_batch():
    import torch
    from dfu3d_amd.pcdet_kitti import centernet_utils
    cfg = dict(ref.CFG_A, point_cloud_range=[-54.0, -54.0, -5.0, 54.0, 54.0, 3.0], voxel_size=[0.075, 0.075, 0.2], stride=8)
    lim = [-50.0, -50.0, -9.0, 50.0, 50.0, 9.0]
    for K, n_cls, B in ((500, 2, 8), (1024, 3, 3), (1, 1, 2)):
        d = ref.decode_inputs(77 + K, B, n_cls, 180, 180, True, True)
        got = run_decode(d, K, 0.5, lim, cfg)
        want = ref.decode_bbox_from_heatmap(d['heatmap'], d['rot_cos'], d['rot_sin'], d['center'], d['center_z'], d['dim'],
                                            cfg['point_cloud_range'], cfg['voxel_size'], cfg['stride'], vel=d['vel'],
                                            iou=d['iou'], K=K, score_thresh=0.5, post_center_limit_range=lim)
        compare_decode(got, want)
    z = torch.zeros((0, 1, 8, 8), device='cuda')
    assert centernet_utils.decode_bbox_from_heatmap(
        z, z, z, torch.zeros((0, 2, 8, 8), device='cuda'), z, torch.zeros((0, 3, 8, 8), device='cuda'),
        point_cloud_range=[0, 0, 0], voxel_size=[1, 1, 1], feature_map_stride=1, K=4,
        post_center_limit_range=[-1, -1, -1, 1, 1, 1]) == []


def test_decode_ties_by_ascending_flat_index():
    """The stated rule only (torch.topk leaves ties unspecified): a constant map returns the first K flat indices in order;
    planted equal pairs come out in ascending flat index; NaN ranks first."""
    H, W, n_cls, K = 128, 64, 2, 500
    HW = H * W
    d = ref.decode_inputs(5, 2, n_cls, H, W, False, True)
    cell = np.arange(HW, dtype=np.float32).reshape(1, 1, H, W)
    d['iou'] = np.broadcast_to(cell, (2, 1, H, W)).copy()                 # pred_iou = the cell of a row, exactly
    lim = [-1e9, -1e9, -1e9, 1e9, 1e9, 1e9]
    d['heatmap'] = np.full((2, n_cls, H, W), 0.10065, np.float32)         # sigmoid(-2.19), an untrained head
    got = run_decode(d, K, None, lim)
    for r in got:
        flat = r['pred_labels'].astype(np.int64) * HW + r['pred_iou'].astype(np.int64)
        assert flat.tolist() == list(range(K))
    # planted equal pairs on a map of distinct scores, and one NaN
    d2 = ref.decode_inputs(6, 2, n_cls, H, W, False, True)
    d2['iou'] = d['iou']
    heat = d2['heatmap'].reshape(2, -1)
    rng = np.random.default_rng(9)
    for b in range(2):
        top = np.argsort(-heat[b], kind='stable')[:200]
        for a, c in rng.permutation(top)[:100].reshape(50, 2):
            heat[b, c] = heat[b, a]
        heat[b, 4321] = np.nan
    d2['heatmap'] = heat.reshape(2, n_cls, H, W)
    got = run_decode(d2, K, None, lim)
    want = ref.decode_bbox_from_heatmap(d2['heatmap'], d2['rot_cos'], d2['rot_sin'], d2['center'], d2['center_z'], d2['dim'],
                                        ref.CFG_A['point_cloud_range'], ref.CFG_A['voxel_size'], ref.CFG_A['stride'],
                                        iou=d2['iou'], K=K, post_center_limit_range=lim)
    for b, (r, w) in enumerate(zip(got, want)):
        flat = r['pred_labels'].astype(np.int64) * HW + r['pred_iou'].astype(np.int64)
        assert flat[0] == 4321 and np.isnan(r['pred_scores'][0])
        assert np.array_equal(flat, w['order'])
        s = r['pred_scores'][1:]
        assert (np.diff(s) <= 0).all()
        ties = np.flatnonzero(np.diff(s) == 0)
        assert len(ties) >= 40 and (flat[1:][ties] < flat[1:][ties + 1]).all()


def _select_case(name):
    """-> (heat maps (2, n_cls, H, W), K): inputs that steer the radix select behind the K-th largest score."""
    n_cls, H, W, K = {'k_equals_n': (1, 8, 8, 64), 'nan_first': (2, 9, 7, 1), 'alone_in_top_byte': (1, 33, 31, 1),
                      'last_byte_only': (1, 16, 16, 100), 'constant': (2, 33, 31, 500)}[name]
    heat = ref.decode_inputs(11, 2, n_cls, H, W, False, True)['heatmap'].reshape(2, -1)
    if name == 'nan_first':                    # the complemented key 0, alone in its bucket in the first pass
        heat[:, 17] = np.nan
    elif name == 'alone_in_top_byte':          # every score below 0.5 but one: the selected key leaves after one pass
        heat *= np.float32(0.49)
        heat[0, 700], heat[1, 3] = 0.75, 0.75
    elif name == 'last_byte_only':             # keys that differ in their last byte only: all four passes
        rs = np.random.RandomState(12)
        heat = np.stack([(0x3E000000 + rs.permutation(256)).astype(np.uint32).view(np.float32) for _ in range(2)])
    elif name == 'constant':                   # 2046 equal keys: every kept row is a tie
        heat[:] = 0.10065
    return np.ascontiguousarray(heat, np.float32).reshape(2, n_cls, H, W), K


@pytest.mark.parametrize("name", ['k_equals_n', 'nan_first', 'alone_in_top_byte', 'last_byte_only', 'constant'])
def test_decode_select_edges_keep_the_stated_order(name):
    """The kept flat indices equal the stated rule's (descending score, ties by ascending flat index, NaN first) where the
    rank is the last one, the selected key is alone in its bucket early or never, and where all keys are equal."""
    heat, K = _select_case(name)
    _, n_cls, H, W = heat.shape
    HW = H * W
    d = ref.decode_inputs(5, 2, n_cls, H, W, False, True)
    d['heatmap'] = heat
    d['iou'] = np.broadcast_to(np.arange(HW, dtype=np.float32).reshape(1, 1, H, W), (2, 1, H, W)).copy()
    lim = [-1e9, -1e9, -1e9, 1e9, 1e9, 1e9]
    got = run_decode(d, K, None, lim)
    want = ref.decode_bbox_from_heatmap(d['heatmap'], d['rot_cos'], d['rot_sin'], d['center'], d['center_z'], d['dim'],
                                        ref.CFG_A['point_cloud_range'], ref.CFG_A['voxel_size'], ref.CFG_A['stride'],
                                        iou=d['iou'], K=K, post_center_limit_range=lim)
    for r, w in zip(got, want):
        flat = r['pred_labels'].astype(np.int64) * HW + r['pred_iou'].astype(np.int64)
        assert len(w['order']) == K and np.array_equal(flat, w['order'])
        assert r['pred_scores'].tobytes() == w['pred_scores'].tobytes()


def test_round_trip_targets_to_predicted_boxes():
    """Independent of the reference: targets from random boxes -> prediction maps written from those targets (a large
    logit at each `inds` cell, the regression maps filled from `target_boxes`) -> generate_predicted_boxes with the config's
    POST_PROCESSING returns every input box with its class, centres and sizes within 1e-3 m and yaw within 1e-3 rad.
    Condition on the input, not a filter on the comparison: boxes are placed on a lattice of 6.4 m (8 cells), so no two
    share a cell, and they are at most 4.5 m long, so no two overlap (NMS keeps all of them)."""
    import torch
    cfg = CFGS["A"]
    H, W = cfg['map_hw']
    rng = np.random.default_rng(33)
    B, n_cls = 4, len(cfg['class_names'])
    gt = np.zeros((B, 100, 8), np.float32)
    for b in range(B):
        sites = [(3.2 + 6.4 * i, -48.0 + 6.4 * j) for i in range(7) for j in range(15)]
        pick = rng.permutation(len(sites))[:60]
        for k, s in enumerate(pick):
            x, y = sites[s]
            gt[b, k] = [x + rng.uniform(-0.3, 0.3), y + rng.uniform(-0.3, 0.3), rng.uniform(-3, 1), rng.uniform(0.5, 4.5),
                        rng.uniform(0.4, 2.0), rng.uniform(0.8, 3.0), rng.uniform(-3.1, 3.1), 1 + rng.integers(n_cls)]
    head = make_head(cfg)
    gt_t = torch.from_numpy(gt).cuda()
    tg = head.assign_targets(gt_t, feature_map_size=[H, W], check=True)
    pred_dicts = []
    for h, names in enumerate(cfg['heads']):
        hm = torch.full((B, len(names), H * W), -10.0, device='cuda')
        reg = torch.zeros((B, 8, H * W), device='cuda')
        inds, masks, tb, src = tg['inds'][h], tg['masks'][h].bool(), tg['target_boxes'][h], tg['target_boxes_src'][h]
        for b in range(B):
            m = masks[b]
            hm[b, (src[b, m, -1] - 1).long(), inds[b, m]] = 10.0
            reg[b][:, inds[b, m]] = tb[b, m].t()
        reg = reg.view(B, 8, H, W)
        pred_dicts.append({'hm': hm.view(B, len(names), H, W), 'center': reg[:, 0:2].contiguous(),
                           'center_z': reg[:, 2:3].contiguous(), 'dim': reg[:, 3:6].contiguous(),
                           'rot': reg[:, 6:8].contiguous()})
    out = head.generate_predicted_boxes(B, pred_dicts)
    for b in range(B):
        boxes, labels = out[b]['pred_boxes'].cpu().numpy(), out[b]['pred_labels'].cpu().numpy()
        real = gt[b][gt[b, :, -1] > 0]
        assert len(boxes) == len(real) == 60
        for g in real:                                                    # every input box, none left out
            d = np.hypot(boxes[:, 0] - g[0], boxes[:, 1] - g[1])
            j = int(np.argmin(d))
            assert labels[j] == int(g[-1])
            assert np.abs(boxes[j, :6] - g[:6]).max() <= 1e-3, (boxes[j], g)
            dyaw = (boxes[j, 6] - g[6] + np.pi) % (2 * np.pi) - np.pi
            assert abs(dyaw) <= 1e-3
        assert (out[b]['pred_scores'] > 0.99).all()
