"""The batched proposal stage on the GPU (csrc/proposal_stage.hip) against tests/proposal_ref.py: the order rule in NumPy
and the existing NMS kernel on boxes already in order.  Integers must be equal, floats equal bit for bit (they are copies
of input rows)."""
import ctypes
import functools
import os

import numpy as np
import pytest

from tests import proposal_ref as P
from tests import roipoint_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
NAMES = ("rois", "roi_scores", "roi_labels", "roi_point_idx", "num_rois")


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(scores, labels, boxes, thresh, pre_max, post_max):
    from dfu3d_amd import proposal_ops as ops
    return [o.cpu().numpy() for o in ops.proposals(cu(scores), cu(labels), cu(boxes), thresh, pre_max, post_max)]


def check(got, exp, what=""):
    for name, g, e in zip(NAMES, got, exp):
        assert g.dtype == e.dtype and g.shape == e.shape, (what, name, g.dtype, g.shape, e.dtype, e.shape)
        assert P.same_bits(g, e), (what, name, np.argwhere(g != e)[:8].tolist())
    assert got[4].dtype == np.int32 and np.array_equal(got[4], (got[3] >= 0).sum(axis=1))


def labels_for(rng, shape):
    return rng.integers(0, 3, shape).astype(np.int64)


# ---- a. block edges ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pre_mode", [-1, 0, 5])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 129, 200])
def test_a_block_edges(N, pre_mode):
    """B = 3, the candidate count at, one short of and beyond the sample (and so at, before and behind the 64-row blocks);
    the stop inside a block (half of the smallest survivor count) and never reached (three beyond the largest)."""
    rng = np.random.default_rng(1000 * N + pre_mode + 7)
    pre = max(N + pre_mode, 1)
    scores, boxes, labels = P.distinct_scores(rng, 3, N), P.clustered_boxes(rng, 3, N), labels_for(rng, (3, N))
    kept = P.walk_ref(scores, boxes, 0.3, pre)
    counts = [len(k) for k in kept]
    print("N %d pre %d survivors %s" % (N, pre, counts))
    assert all(1 <= c <= min(pre, N) for c in counts)
    if N >= 63:
        assert all(c < min(pre, N) for c in counts) and max(counts) > 6          # suppression is common, not total
    for post in sorted({max(min(counts) // 2, 1), max(counts) + 3}):
        check(run(scores, labels, boxes, 0.3, pre, post), P.pad_ref(kept, scores, labels, boxes, post), "post %d" % post)


def _with_copies(n, copies, C=7):
    """n disjoint boxes in walk order, the positions in `copies` copies of position 0 -> rows, kept positions."""
    rows = P.disjoint_boxes(n, C)
    rows[list(copies)] = rows[0]
    return rows, np.setdiff1d(np.arange(n), list(copies))


@pytest.mark.parametrize("last", [63, 127])
def test_a_stop_on_the_last_row_of_a_block(last):
    """Keep lists known by construction.  Sample 0: three copies of row 0 before `last`, so row `last` -- the last of its
    block of 64 -- is the post_max-th kept; sample 1: two copies, the stop falls one row earlier, inside the block; sample
    2: all rows equal, one survivor."""
    rng = np.random.default_rng(last)
    n, post = 200, last + 1 - 3
    cases = [_with_copies(n, (10, 20, 30)), _with_copies(n, (5, 40)), (np.repeat(P.disjoint_boxes(1), n, 0), np.array([0]))]
    parts = [P.by_position(rng, rows) for rows, _ in cases]
    scores, boxes = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    labels = labels_for(rng, scores.shape)
    got = run(scores, labels, boxes, 0.5, n, post)
    assert got[4].tolist() == [post, post, 1]
    for b, ((_, keep), (_, _, perm)) in enumerate(zip(cases, parts)):
        exp = perm[keep[:post]]
        assert np.array_equal(got[3][b, :len(exp)], exp) and (got[3][b, len(exp):] == -1).all(), b
    assert got[3][0, post - 1] == parts[0][2][last] and got[3][1, post - 1] == parts[1][2][last - 1]
    check(got, P.proposals_ref(scores, labels, boxes, 0.5, n, post))


# ---- b. hand patterns ----------------------------------------------------------------------------------------------------
def test_b_all_identical_and_all_disjoint():
    rng = np.random.default_rng(2)
    scores, boxes, perm = P.by_position(rng, np.repeat(P.disjoint_boxes(1), 200, 0))
    labels = labels_for(rng, scores.shape)
    got = run(scores, labels, boxes, 0.5, 9000, 70)
    assert got[4].tolist() == [1] and got[3][0, 0] == perm[0] and (got[3][0, 1:] == -1).all()
    assert not got[0][0, 1:].any() and not got[1][0, 1:].any() and (got[2][0, 1:] == 1).all()
    assert got[2][0, 0] == labels[0, perm[0]] + 1 and got[1][0, 0] == scores[0, perm[0]]
    # disjoint: exactly the first 70 in order
    scores, boxes, perm = P.by_position(rng, P.disjoint_boxes(300, 9))
    boxes[..., 7:] = rng.normal(0, 1, (1, 300, 2))
    labels = labels_for(rng, scores.shape)
    got = run(scores, labels, boxes, 0.5, 300, 70)
    assert got[4].tolist() == [70] and np.array_equal(got[3][0], perm[:70])
    assert P.same_bits(got[0][0], boxes[0][perm[:70]]) and P.same_bits(got[1][0], scores[0][perm[:70]])
    assert np.array_equal(got[2][0], labels[0][perm[:70]] + 1)


@pytest.mark.parametrize("p", [0, 63, 127])
def test_b_chain_across_a_block_edge(p):
    """2 x 1 boxes one metre apart at positions p, p + 1, p + 2 (IoU 1/3 between neighbours, the outer two only touch):
    p suppresses p + 1, and p + 2 -- which only the suppressed p + 1 overlaps -- is kept."""
    rng = np.random.default_rng(p)
    n = 200
    rows = P.disjoint_boxes(n)
    rows[p + 1], rows[p + 2] = rows[p], rows[p]
    rows[p + 1, 0] += 1.0
    rows[p + 2, 0] += 2.0
    scores, boxes, perm = P.by_position(rng, rows)
    labels = labels_for(rng, scores.shape)
    got = run(scores, labels, boxes, 0.25, n, 512)
    keep = np.setdiff1d(np.arange(n), [p + 1])
    assert got[4].tolist() == [n - 1] and np.array_equal(got[3][0, :n - 1], perm[keep]) and (got[3][0, n - 1:] == -1).all()
    check(got, P.proposals_ref(scores, labels, boxes, 0.25, n, 512))


# ---- c. ties ----------------------------------------------------------------------------------------------------------
def test_c_ties_follow_the_order_rule():
    """Four distinct values, -0.0 and +0.0 among them (one key): any order but (key, ascending index) changes the result.
    pre_max cuts inside a run of equal keys."""
    rng = np.random.default_rng(3)
    B, N = 2, 300
    scores = rng.choice(np.array([-0.0, 0.0, 1.5, -2.0], f32), (B, N))
    assert np.signbit(scores[scores == 0]).any() and not np.signbit(scores[scores == 0]).all()
    boxes, labels = P.clustered_boxes(rng, B, N), labels_for(rng, (B, N))
    for pre, post in ((250, 40), (300, 300), (100, 7)):
        exp = P.proposals_ref(scores, labels, boxes, 0.3, pre, post)
        assert exp[4].min() > 3
        check(run(scores, labels, boxes, 0.3, pre, post), exp, "pre %d post %d" % (pre, post))
    key, full = P.sort_key(scores[0]), P.order_ref(scores[0], N)
    assert key[full[249]] == key[full[250]] and key[full[99]] == key[full[100]]                  # the cuts are inside ties


# ---- d. beyond the old cap -----------------------------------------------------------------------------------------------
def test_d_more_candidates_than_the_segmented_nms_takes():
    from dfu3d_amd import _lib_post
    B, N, pre, post = 2, 3000, 2500, 512
    assert pre > _lib_post.CONSTANTS["DFU3D_POST_MAX_CAP"]
    # tight clusters: fewer than post_max survive, the walk visits all 2 500 candidates
    rng = np.random.default_rng(41)
    scores, labels = P.distinct_scores(rng, B, N), labels_for(rng, (B, N))
    boxes = P.clustered_boxes(rng, B, N, centres=40, jitter=0.06)
    kept = P.walk_ref(scores, boxes, 0.8, pre)
    print("tight: survivors", [len(k) for k in kept])
    assert all(40 <= len(k) < post for k in kept)
    check(run(scores, labels, boxes, 0.8, pre, post), P.pad_ref(kept, scores, labels, boxes, post), "tight")
    # loose: 512 are kept long before the candidates run out
    boxes = P.clustered_boxes(rng, B, N, centres=40, jitter=0.4, scattered=0.6)
    kept = P.walk_ref(scores, boxes, 0.8, pre)
    print("loose: survivors", [len(k) for k in kept])
    assert all(len(k) > post + 100 for k in kept)
    exp = P.pad_ref(kept, scores, labels, boxes, post)
    assert exp[4].tolist() == [post] * B
    check(run(scores, labels, boxes, 0.8, pre, post), exp, "loose")


# ---- e. against the per-sample layer -----------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["TRAIN", "TEST"])
@pytest.mark.parametrize("C", [7, 9])
def test_e_batched_layer_equals_the_per_sample_layer(C, mode):
    import torch
    from dfu3d_amd.pcdet_kitti.pointrcnn_head import PointRCNNHead
    rng = np.random.default_rng(50 + C)
    B, N = 4, 512
    nms = R.full_model_cfg()['ROI_HEAD']['NMS_CONFIG'][mode]
    assert (nms['NMS_PRE_MAXSIZE'], nms['NMS_POST_MAXSIZE'], nms['NMS_THRESH']) == \
        ((9000, 512, 0.8) if mode == "TRAIN" else (9000, 100, 0.85))
    best = P.distinct_scores(rng, B, N)                       # distinct per sample: torch.topk has no tie
    cls = (best[..., None] - 1.0 - rng.uniform(0, 1, (B, N, 3))).astype(f32)
    col = rng.integers(0, 3, (B, N))
    np.put_along_axis(cls, col[..., None], best[..., None], axis=2)
    boxes = P.clustered_boxes(rng, B, N, C=C, centres=12, jitter=0.15, scattered=0.3)
    head = PointRCNNHead(16, R.g20_model_cfg()['ROI_HEAD'], num_class=1, batched_proposals=True)
    src = {'batch_size': B, 'batch_cls_preds': cu(cls.reshape(B * N, 3)), 'batch_box_preds': cu(boxes.reshape(B * N, C)),
           'batch_index': cu(np.repeat(np.arange(B), N).astype(f32))}
    one, two = head.proposal_layer(dict(src), nms), head.proposal_layer_batched(dict(src), nms)
    assert sorted(two) == sorted(list(one) + ['num_rois']) and 'batch_index' not in two
    assert one['has_class_labels'] is True and two['has_class_labels'] is True
    for key in ('rois', 'roi_scores', 'roi_labels', 'roi_point_idx'):
        assert one[key].dtype == two[key].dtype and torch.equal(one[key], two[key]), key
    assert two['num_rois'].dtype == torch.int32 and torch.equal(two['num_rois'].long(), (two['roi_point_idx'] >= 0).sum(dim=1))
    n = two['num_rois'].tolist()
    print(mode, C, "survivors", n)
    assert min(n) > 20 and (mode == "TEST" or min(n) < 512)
    assert np.array_equal(two['roi_labels'].cpu().numpy()[0, :n[0]], col[0][two['roi_point_idx'].cpu().numpy()[0, :n[0]]] + 1)


# ---- f. golden G20 through the batched layer -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def g20(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g20_pointrcnn.npz")))


def _g20_model(g, **kw):
    import json
    import torch
    from dfu3d_amd.pcdet_kitti.point_rcnn import PointRCNN
    model = PointRCNN(R.g20_model_cfg(), len(R.G20_CLASSES), class_names=R.G20_CLASSES, num_point_features=3 + R.G20_EXTRA, **kw)
    keys = json.loads(bytes(g["meta"]).decode())["state_dict_keys"]
    model.load_state_dict({k: torch.from_numpy(g["sd_" + k].copy()) for k in keys}, strict=True)
    return model.to(DEV).eval()


def test_f_golden_g20(g20):
    import torch
    model, plain = _g20_model(g20, batched_proposals=True), _g20_model(g20)
    assert model.roi_head.batched_proposals and not plain.roi_head.batched_proposals
    cfg = R.g20_model_cfg()
    d = {'batch_size': R.G20_B, 'batch_cls_preds': cu(g20["point_cls_preds"]), 'batch_box_preds': cu(g20["stage1_boxes"]),
         'batch_index': cu(g20["point_coords"])[:, 0]}
    model.roi_head.proposal_layer_batched(d, nms_config=cfg['ROI_HEAD']['NMS_CONFIG']['TEST'])
    assert np.array_equal(d['roi_point_idx'].cpu().numpy(), g20["roi_point_idx"])
    assert np.array_equal(d['roi_labels'].cpu().numpy(), g20["roi_labels"]) and d['roi_labels'].dtype == torch.int64
    assert np.array_equal(d['rois'].cpu().numpy(), g20["rois"]) and np.array_equal(d['roi_scores'].cpu().numpy(), g20["roi_scores"])
    assert d['has_class_labels'] is True and 'batch_index' not in d
    assert d['num_rois'].tolist() == (g20["roi_point_idx"] >= 0).sum(axis=1).tolist()
    with torch.no_grad():
        got, recall = model(dict(points=cu(g20["points"]), batch_size=R.G20_B))
        exp, _ = plain(dict(points=cu(g20["points"]), batch_size=R.G20_B))
    assert recall == {} and len(got) == len(exp) == R.G20_B
    assert [len(p['pred_scores']) for p in got] == g20["pred_count"].tolist()
    for a, b in zip(got, exp):
        for key in ('pred_boxes', 'pred_scores', 'pred_labels'):
            assert a[key].dtype == b[key].dtype and torch.equal(a[key], b[key]), key


# ---- g. launches and host reads ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _plain_case(B, N=700):
    rng = np.random.default_rng(60 + B)
    return (P.distinct_scores(rng, B, N), labels_for(rng, (B, N)),
            P.clustered_boxes(rng, B, N, C=8, centres=10, jitter=0.3, scattered=0.2))


def test_g_launch_count(monkeypatch):
    import torch
    from dfu3d_amd import _lib, _lib_prop, proposal_ops as ops
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib, "_LIB", L)
    monkeypatch.setattr(_lib_prop, "_BOUND", _lib_prop.bind(L))
    assert 1 <= ops.LAUNCHES <= 3
    for B in (1, 5):
        scores, labels, boxes = (cu(a) for a in _plain_case(B))
        L.dfu3d_debug_launch_count(1)
        out = ops.proposals(scores, labels, boxes, 0.5, 600, 100)
        assert int(L.dfu3d_debug_launch_count(1)) == ops.LAUNCHES, B
        torch.cuda.synchronize()
        check([o.cpu().numpy() for o in out], P.proposals_ref(*_plain_case(B), 0.5, 600, 100), "count build, B %d" % B)


def test_g_no_host_read():
    import torch
    from dfu3d_amd import proposal_ops as ops
    scores, labels, boxes = (cu(a) for a in _plain_case(5))
    ops.proposals(scores, labels, boxes, 0.5, 600, 100)           # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.proposals(scores, labels, boxes, 0.5, 600, 100)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(out[4].sum()) > 0


# ---- h. determinism and robustness -----------------------------------------------------------------------------------------
def test_h_twice_and_on_a_side_stream():
    import torch
    from dfu3d_amd import proposal_ops as ops
    scores, labels, boxes = (cu(a) for a in _plain_case(5))
    first = ops.proposals(scores, labels, boxes, 0.5, 600, 100)
    second = ops.proposals(scores, labels, boxes, 0.5, 600, 100)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = ops.proposals(scores, labels, boxes, 0.5, 600, 100)
    side.synchronize()
    torch.cuda.synchronize()
    for a, b, c in zip(first, second, third):
        assert P.same_bits(a.cpu().numpy(), b.cpu().numpy()) and P.same_bits(a.cpu().numpy(), c.cpu().numpy())
    check([o.cpu().numpy() for o in first], P.proposals_ref(*_plain_case(5), 0.5, 600, 100))


def test_h_nan_scores_and_boxes_without_extent():
    """Ordinary inputs to the order rule and to rect_area: a NaN score ranks first, a box of zero extent has IoU 0 with
    everything (it suppresses nothing and nothing suppresses it), a NaN box is in no pair."""
    rng = np.random.default_rng(8)
    B, N = 2, 300
    scores, labels, boxes = P.distinct_scores(rng, B, N), labels_for(rng, (B, N)), P.clustered_boxes(rng, B, N)
    scores[0, 17] = scores[1, 250] = np.nan
    scores[1, 3] = np.array([0xFFC00000], np.uint32).view(f32)[0]          # a NaN with the sign bit
    scores[0, 5], scores[0, 6] = np.inf, -np.inf
    boxes[0, 17, 3:6] = 0                                                   # the NaN-scored point has no extent
    boxes[0, 40, 3] = 0
    boxes[1, 60, 3:5] = 0
    boxes[1, 61] = boxes[1, 60]                                             # two equal boxes of no extent: both stay
    scores[1, 60], scores[1, 61] = 2.5, 2.4                                # (no other point has these scores)
    boxes[1, 250, 0:2] = 500.0                                              # the second NaN score: away from the first
    boxes[1, 90, 0] = np.nan
    boxes[1, 91, 6] = np.inf
    exp = P.proposals_ref(scores, labels, boxes, 0.3, 280, 200)
    got = run(scores, labels, boxes, 0.3, 280, 200)
    check(got, exp)
    assert got[3][0, :2].tolist() == [17, 5] and got[3][1, :2].tolist() == [3, 250]
    assert np.isnan(got[1][0, 0]) and {60, 61} <= set(got[3][1].tolist())


@pytest.mark.parametrize("thresh", [-1.0, 0.0, 2.0, float('nan')])
def test_h_thresholds_at_and_beyond_the_ends(thresh):
    """thresh < 0: a pair without any overlap suppresses too, so one box per sample survives; thresh = 0: any overlap
    suppresses; thresh >= 1 or NaN: nothing does, the kept list grows by 64 a block and the candidates meet it in full."""
    rng = np.random.default_rng(9)
    B, N = 2, 300
    scores, labels, boxes = P.distinct_scores(rng, B, N), labels_for(rng, (B, N)), P.clustered_boxes(rng, B, N, C=8)
    exp = P.proposals_ref(scores, labels, boxes, thresh, 290, 130)
    want = [1, 1] if thresh < 0 else ([130, 130] if thresh != 0 else None)
    assert want is None or exp[4].tolist() == want
    assert thresh != 0 or (1 < exp[4].min() and exp[4].max() < 60)
    check(run(scores, labels, boxes, thresh, 290, 130), exp, "thresh %r" % thresh)
