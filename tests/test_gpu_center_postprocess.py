"""GPU: row f-9, the CenterHead post-processing for a whole batch on csrc/postproc_stage.hip -- the segmented NMS
(stages.nms_bev_segments / dfu3d_nms_bev_segments), the gather (dfu3d_center_collect) and
CenterHead.generate_predicted_boxes_batched.

Expected keep lists come from oracle/iou3d_oracle.py (pair_ious, widest_gap_threshold, nms_sparse) and, end to end, from
the existing per-sample path `generate_predicted_boxes`; never from the code under test.  The thresholds of the oracle
cases sit in the middle of the widest gap between oracle IoU values near 0.2, with a half-width above 1e-5 (the margin
tests/test_gpu_iou3d.py established for this clipper), so no pair is ambiguous.  Seeds: the segment scene is the first
seed tried (SCENE_SEED); the end-to-end maps are the first seed tried (E2E_SEED) -- their scores are distinct by
construction and the test asserts it on the decoded rows."""
import ctypes

import numpy as np
import pytest

from oracle import iou3d_oracle as oracle
from tests import center_head_ref as ref
from tests.iou3d_cases import random_boxes

pytestmark = pytest.mark.gpu
f32 = np.float32
DEV = "cuda:0"
CAP = 1024
COUNTS = [0, 1, 63, 64, 65, 500, 1000, 1024]
SCENE_SEED = 909
E2E_SEED = 4242
MARGIN = 1e-5


# ---- the segment scene and the oracle's answers (computed once, never changed) -----------------------------------------
def _spread(n):
    """Half side of the square the n boxes of a segment fall on: about 5 m^2 of ground per box of about 11 m^2."""
    return 1.1 * np.sqrt(max(n, 1))


@pytest.fixture(scope="module")
def scene():
    rng = np.random.default_rng(SCENE_SEED)
    lists = [random_boxes(rng, n, _spread(n)) for n in COUNTS]
    out = {"lists": lists}
    for normal in (False, True):
        pairs = [oracle.pair_ious(b, normal=normal) for b in lists]
        thresh, half = oracle.widest_gap_threshold(np.concatenate([p[2] for p in pairs]), 0.2)
        assert half > MARGIN, (normal, half)
        assert all((np.abs(p[2] - thresh) > MARGIN).all() for p in pairs)
        keeps = [oracle.nms_sparse(b, -np.arange(len(b), dtype=np.float64), thresh, normal=normal, pairs=p)[0]
                 for b, p in zip(lists, pairs)]
        for n, k in zip(COUNTS, keeps):
            if n >= 63:                                                   # a trivial walk cannot pass
                assert 0.2 * n <= n - len(k) <= 0.8 * n, (normal, n, len(k))
        out[normal] = (f32(thresh), keeps)
        assert abs(float(f32(thresh)) - thresh) < 0.1 * MARGIN
    return out


def _block(lists, C=7, cap=CAP, fill=None, seed=5):
    """(S, cap, C) float32: the lists at the head of their segments; behind them `fill` ('nan', 'row0' or zeros);
    columns 7.. are noise."""
    rng = np.random.default_rng(seed)
    S = len(lists)
    b = np.zeros((S, cap, C), f32)
    if fill == "nan":
        b[:] = np.nan
    for s, rows in enumerate(lists):
        if fill == "row0" and len(rows):
            b[s, :, :7] = rows[0]
        b[s, :len(rows), :7] = rows
    if C > 7:
        b[:, :, 7:] = rng.uniform(-50, 50, (S, cap, C - 7))
    return b


def _run(boxes, counts, thresh, pre_max=None, post_max=None, normal=False):
    import torch
    from dfu3d_amd import stages
    keep, num = stages.nms_bev_segments(torch.from_numpy(boxes).to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV),
                                        float(thresh), pre_max=pre_max, post_max=post_max, normal=normal)
    assert keep.dtype == torch.int32 and num.dtype == torch.int32 and tuple(keep.shape) == boxes.shape[:2]
    return keep.cpu().numpy(), num.cpu().numpy()


def _check(keep, num, expected, what=""):
    for s, want in enumerate(expected):
        want = np.asarray(want, np.int64)
        assert num[s] == len(want), (what, s, int(num[s]), len(want))
        assert np.array_equal(keep[s, :len(want)], want), (what, s, np.setxor1d(keep[s, :len(want)], want)[:16])
        assert (keep[s, len(want):] == -1).all(), (what, s)


# ---- 1 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [7, 9])
@pytest.mark.parametrize("normal", [False, True])
def test_segments_match_the_oracle(scene, C, normal):
    thresh, keeps = scene[normal]
    keep, num = _run(_block(scene["lists"], C=C), COUNTS, thresh, normal=normal)
    _check(keep, num, keeps, "C=%d normal=%s" % (C, normal))


# ---- 2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fill", ["nan", "row0"])
def test_segments_do_not_leak_and_padding_is_not_read(scene, fill):
    thresh, keeps = scene[False]
    pick = [5, 5, 7, 0, 6, 6, 3]                                           # 500, 500, 1024, 0, 1000, 1000, 64 rows
    lists = [scene["lists"][k] for k in pick]
    counts = [COUNTS[k] for k in pick]
    counts[2], counts[3] = CAP + 5, -3
    blk = _block(lists, fill=fill)
    if fill == "row0":
        blk[3, :, :7] = scene["lists"][5][0]                               # the empty segment holds boxes too
    keep, num = _run(blk, counts, thresh)
    _check(keep, num, [keeps[k] for k in pick], fill)


# ---- 3 ----------------------------------------------------------------------------------------------------------------
def test_pre_and_post_cuts(scene):
    thresh, keeps = scene[False]
    lists = [scene["lists"][k] for k in (5, 6, 7, 4)]                      # 500, 1000, 1024, 65 rows
    counts = [len(b) for b in lists]
    blk = _block(lists)
    n_kept = min(len(keeps[k]) for k in (5, 6, 7))
    for pre, post in ((300, None), (None, n_kept // 2), (300, 40), (64, None), (65, 1), (2000, 5000)):
        want = []
        for b in lists:
            k = oracle.nms_sparse(b, -np.arange(len(b), dtype=np.float64), float(thresh), pre_maxsize=pre)[0]
            want.append(k[:post] if post is not None else k)
        if pre == 300:
            assert all(len(b) > pre for b in lists[:3])
        if post is not None and post < 1000:
            assert all(len(w) == post for w in want[:3])                  # the cut is below the kept number
        keep, num = _run(blk, counts, thresh, pre_max=pre, post_max=post)
        _check(keep, num, want, "pre=%s post=%s" % (pre, post))


# ---- 4 ----------------------------------------------------------------------------------------------------------------
STRICT_PAIRS = [(0, 1), (2, 63), (3, 64), (5, 127), (6, 128), (7, 1023)]


def _strict_scene():
    """Disjoint 2 x 1 boxes on a 4 m lattice, heading 0, power-of-two coordinates; box j of a pair is the 1 x 1 box inside
    the 2 x 1 box i: overlap 1, union 2, IoU exactly 0.5 in float32."""
    k = np.arange(CAP)
    b = np.zeros((CAP, 7), f32)
    b[:, 0], b[:, 1] = 8.0 + 4.0 * (k % 256), 8.0 + 4.0 * (k // 256)
    b[:, 3], b[:, 4], b[:, 5] = 2.0, 1.0, 1.0
    for i, j in STRICT_PAIRS:
        b[j] = b[i]
        b[j, 0] += f32(0.5)
        b[j, 3] = 1.0
    return b


@pytest.mark.parametrize("normal", [False, True])
def test_threshold_is_strict_on_word_boundaries(normal):
    blk = _block([_strict_scene(), _strict_scene()[:500]])
    every = [np.arange(CAP), np.arange(500)]
    keep, num = _run(blk, [CAP, 500], f32(0.5), normal=normal)
    _check(keep, num, every, "IoU == thresh")
    below = np.nextafter(f32(0.5), f32(0))
    assert float(below) < 0.5
    inner = [j for _, j in STRICT_PAIRS]
    keep, num = _run(blk, [CAP, 500], below, normal=normal)
    _check(keep, num, [np.setdiff1d(every[0], inner), np.setdiff1d(every[1], inner)], "one float32 below")


# ---- 5: end to end ------------------------------------------------------------------------------------------------------
def _post(post_max):
    return dict(SCORE_THRESH=0.1, POST_CENTER_LIMIT_RANGE=[0, -61.2, -10.0, 61.2, 61.2, 10.0], MAX_OBJ_PER_SAMPLE=500,
                NMS_CONFIG=dict(MULTI_CLASSES_NMS=True, NMS_TYPE='nms_gpu', NMS_THRESH=0.6, NMS_PRE_MAXSIZE=1000,
                                NMS_POST_MAXSIZE=post_max))


def make_head(post, vel=False, **over):
    from dfu3d_amd.pcdet_kitti.center_head import CenterHead
    c = ref.CFG_A
    model_cfg = dict(CLASS_NAMES_EACH_HEAD=c['heads'], POST_PROCESSING=dict(post, **over),
                     SEPARATE_HEAD_CFG=dict(HEAD_ORDER=['center', 'center_z', 'dim', 'rot'] + (['vel'] if vel else [])),
                     TARGET_ASSIGNER_CONFIG=dict(FEATURE_MAP_STRIDE=c['stride'], NUM_MAX_OBJS=c['num_max_objs'],
                                                 GAUSSIAN_OVERLAP=c['gaussian_overlap'], MIN_RADIUS=c['min_radius']))
    return CenterHead(model_cfg, c['class_names'], np.array(c['point_cloud_range'], np.float32), c['voxel_size'])


# cells above the score threshold per (head, sample): -1 = hm is -10 everywhere
ABOVE = [[420, 700, 60], [300, -1, 1], [150, -1, 500], [90, 250, 380], [640, 30, 200], [500, 120, 330]]


def e2e_maps(seed=E2E_SEED, B=3, vel=False, above=None):
    """Random prediction maps of config A's six heads (NumPy, logits).  Of head h, sample b, above[h][b] (ABOVE) cells carry
    distinct logits in [-2, 3] (scores above SCORE_THRESH = 0.1: sigmoid(-2) = 0.119), placed at random over the classes
    within a band of the map of about 9 cells per box; all others are distinct values in [-9, -3].  The logits of a
    (head, sample) are an arithmetic progression of step >= 2e-4, so their sigmoids differ by far more than a float32
    step: the scores are pairwise distinct.  dim = log(7) +- 4 %, headings within 0.05 rad of 0: boxes of 7 m on a
    0.8 m lattice overlap their neighbours above IoU 0.6."""
    rng = np.random.default_rng(seed)
    above = ABOVE if above is None else above
    H, W = ref.CFG_A['map_hw']
    HW = H * W
    preds = []
    for h, names in enumerate(ref.CFG_A['heads']):
        n_cls = len(names)
        N = n_cls * HW
        hm = np.empty((B, N), f32)
        for b in range(B):
            m = above[h][b]
            if m < 0:
                hm[b] = -10.0
                continue
            band = min(H, max(2, (9 * m) // (W * n_cls) + 1)) * W            # cells of the band per class
            cand = np.concatenate([c * HW + np.arange(band) for c in range(n_cls)])
            hot = rng.permutation(cand)[:m]
            cold = np.setdiff1d(np.arange(N), hot)
            hm[b, rng.permutation(hot)] = np.linspace(-2.0, 3.0, m + 1)[1:]
            hm[b, rng.permutation(cold)] = np.linspace(-9.0, -3.0, cold.size)
        d = {'hm': hm.reshape(B, n_cls, H, W),
             'center': rng.uniform(0.0, 1.0, (B, 2, H, W)).astype(f32),
             'center_z': rng.uniform(-3, 1, (B, 1, H, W)).astype(f32),
             'dim': (np.log(7.0) + rng.uniform(-0.04, 0.04, (B, 3, H, W))).astype(f32),
             'rot': np.stack([rng.uniform(0.9, 1.1, (B, H, W)), rng.uniform(-0.05, 0.05, (B, H, W))], 1).astype(f32)}
        if vel:
            d['vel'] = rng.uniform(-5, 5, (B, 2, H, W)).astype(f32)
        preds.append(d)
    return preds


def _to_dev(preds):
    import torch
    return [{k: torch.from_numpy(v).to(DEV) for k, v in d.items()} for d in preds]


def _decoded(head, dev):
    """Scores and counts of the decode alone per (head, sample), through the existing decode_raw."""
    import torch
    from dfu3d_amd.pcdet_kitti import centernet_utils
    post = head.model_cfg['POST_PROCESSING']
    out = []
    for d in dev:
        _, scores, _, _, count = centernet_utils.decode_raw(
            d['hm'].sigmoid(), d['rot'][:, 0:1], d['rot'][:, 1:2], d['center'], d['center_z'], d['dim'].exp(),
            head.point_cloud_range, head.voxel_size, head.feature_map_stride, vel=d.get('vel'), K=post['MAX_OBJ_PER_SAMPLE'],
            score_thresh=post['SCORE_THRESH'],
            post_center_limit_range=torch.tensor(post['POST_CENTER_LIMIT_RANGE'], dtype=torch.float32, device=DEV))
        out.append([scores[b, :n].cpu().numpy() for b, n in enumerate(count.tolist())])
    return out


@pytest.mark.parametrize("post_max,vel", [(83, False), (500, False), (83, True)])
def test_batched_equals_the_per_sample_path(post_max, vel):
    import torch
    B = 3
    head = make_head(_post(post_max), vel=vel)
    dev = _to_dev(e2e_maps(vel=vel))
    dec = _decoded(head, dev)
    # conditions on the input
    for h in range(6):
        for b in range(B):
            s = dec[h][b]
            assert np.unique(s).size == s.size, (h, b)                    # pairwise distinct scores
            if ABOVE[h][b] < 0:
                assert s.size == 0
    assert dec[1][2].size == 1
    want = head.generate_predicted_boxes(B, dev)                          # the comparator
    # NMS does real work: seen on the comparator without the post cut in the way
    uncut = want if post_max >= 500 else make_head(_post(500), vel=vel).generate_predicted_boxes(B, dev)
    real = 0
    pairs = [(h, b) for h in range(6) for b in range(B) if dec[h][b].size > 0]
    for h, b in pairs:
        ids = [ref.CFG_A['class_names'].index(x) + 1 for x in ref.CFG_A['heads'][h]]
        left = int(np.isin(uncut[b]['pred_labels'].cpu().numpy(), ids).sum())
        n = dec[h][b].size
        real += 0.2 * n <= n - left <= 0.8 * n
    assert 2 * real >= len(pairs), (real, len(pairs))
    got = head.generate_predicted_boxes_batched(B, dev)
    pad = head.generate_predicted_boxes_batched(B, dev, as_padded=True)
    C = 9 if vel else 7
    out_cap = 6 * min(500, post_max)
    assert tuple(pad['pred_boxes'].shape) == (B, out_cap, C) and pad['count'].dtype == torch.int32
    assert pad['pred_labels'].dtype == torch.int64 and tuple(pad['pred_scores'].shape) == (B, out_cap)
    counts = pad['count'].tolist()
    assert len(got) == len(want) == B
    for b in range(B):
        n = counts[b]
        assert n == want[b]['pred_scores'].shape[0] and n > 0
        for key in ('pred_boxes', 'pred_scores', 'pred_labels'):
            w = want[b][key].cpu().numpy()
            g, p = got[b][key].cpu().numpy(), pad[key][b].cpu().numpy()
            assert g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes(), (b, key)
            assert p[:n].tobytes() == w.tobytes(), (b, key)
            assert not p[n:].any(), (b, key)                              # rows beyond count are 0
        assert got[b]['pred_labels'].dtype == torch.int64 and got[b]['pred_boxes'].shape[1] == C


# ---- 6 ----------------------------------------------------------------------------------------------------------------
def test_padded_form_makes_no_synchronisation():
    """torch's sync debug mode raises on any synchronising call of torch's own; the library itself never synchronises."""
    import torch
    head = make_head(_post(83))
    dev = _to_dev(e2e_maps())
    head.generate_predicted_boxes_batched(3, dev, as_padded=True)         # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pad = head.generate_predicted_boxes_batched(3, dev, as_padded=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert int(pad['count'].sum()) > 0


# ---- 7 ----------------------------------------------------------------------------------------------------------------
def test_launch_counts(scene, monkeypatch):
    """In the build that counts every kernel launch of the library: NMS + collect cost at most 3 launches for 6 and for
    384 segments; the whole batched call costs those plus the decode's own launches per head."""
    import torch
    from dfu3d_amd import _lib, _lib_post, stages
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib, "_LIB", L)
    monkeypatch.setattr(_lib_post, "_BOUND", _lib_post.bind(L))
    rng = np.random.default_rng(3)
    for n_heads, B, cap in ((6, 1, 500), (6, 64, 200)):
        S = n_heads * B
        boxes = torch.from_numpy(np.stack([random_boxes(rng, cap, 12.0) for _ in range(S)])).to(DEV)
        count = torch.full((S,), cap, dtype=torch.int32, device=DEV)
        scores = torch.rand((S, cap), device=DEV)
        labels = torch.zeros((S, cap), dtype=torch.int32, device=DEV)
        cls_map = torch.zeros((n_heads, 2), dtype=torch.int32, device=DEV)
        L.dfu3d_debug_launch_count(1)
        keep, num = stages.nms_bev_segments(boxes, count, 0.2, pre_max=1000, post_max=83)
        stages.center_collect(boxes.view(n_heads, B, cap, 7), scores, labels, keep, num, cls_map, n_heads * 83)
        n = int(L.dfu3d_debug_launch_count(1))
        assert 0 < n <= 3, (S, n)
    head = make_head(_post(83))
    dev = _to_dev(e2e_maps())
    L.dfu3d_debug_launch_count(1)
    _decoded(head, dev[:1])
    per_decode = int(L.dfu3d_debug_launch_count(1))
    assert per_decode >= 1
    head.generate_predicted_boxes_batched(3, dev, as_padded=True)
    whole = int(L.dfu3d_debug_launch_count(1))
    torch.cuda.synchronize()
    assert whole <= 3 + 6 * per_decode, (whole, per_decode)


# ---- 8 ----------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(scene):
    thresh, _ = scene[False]
    blk = _block(scene["lists"])
    a, b = _run(blk, COUNTS, thresh), _run(blk, COUNTS, thresh)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    head = make_head(_post(83))
    dev = _to_dev(e2e_maps())
    p, q = (head.generate_predicted_boxes_batched(3, dev, as_padded=True) for _ in range(2))
    for key in p:
        assert p[key].cpu().numpy().tobytes() == q[key].cpu().numpy().tobytes(), key


# ---- 9 ----------------------------------------------------------------------------------------------------------------
def test_unsupported_configurations_raise_before_any_launch(monkeypatch):
    import torch
    from dfu3d_amd import _lib, _lib_post
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib, "_LIB", L)
    monkeypatch.setattr(_lib_post, "_BOUND", _lib_post.bind(L))
    dev = _to_dev(e2e_maps())
    with_iou = [dict(d, iou=torch.zeros_like(d['center_z'])) for d in dev]
    cases = []
    for nms_type in ('class_specific_nms', 'circle_nms'):
        post = _post(83)
        post['NMS_CONFIG'] = dict(post['NMS_CONFIG'], NMS_TYPE=nms_type)
        cases.append((make_head(post), dev))
    cases.append((make_head(_post(83), USE_IOU_TO_RECTIFY_SCORE=True, IOU_RECTIFIER=[0.5] * 10), dev))
    cases.append((make_head(_post(83)), with_iou))
    cases.append((make_head(_post(83), MAX_OBJ_PER_SAMPLE=[500, 500, 200, 500, 500, 500]), dev))
    L.dfu3d_debug_launch_count(1)
    for head, preds in cases:
        for padded in (False, True):
            with pytest.raises(NotImplementedError):
                head.generate_predicted_boxes_batched(3, preds, as_padded=padded)
    assert int(L.dfu3d_debug_launch_count(1)) == 0
