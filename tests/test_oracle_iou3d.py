"""f-3 oracle (overlap of rotated boxes / IoU criteria / NMS, float64 world-frame clipping) against geometry:
analytic overlaps, invariances, and a brute-force area estimate on a fine grid.  CPU only."""
import numpy as np

from oracle import iou3d_oracle as I


def test_analytic_cases():
    A = np.array([[0, 0, 0, 4, 2, 1.5, 0.0]])
    assert abs(I.boxes_bev(A, A)[0, 0] - 1.0) < 1e-12                                  # identical
    B = np.array([[2, 0, 0, 4, 2, 1.5, 0.0]])                                         # shifted by half its length
    assert abs(I.boxes_bev(A, B, iou=False)[0, 0] - 4.0) < 1e-12
    assert abs(I.boxes_bev(A, B)[0, 0] - 4.0 / 12.0) < 1e-12
    C = np.array([[10, 10, 0, 4, 2, 1.5, 0.3]])                                        # disjoint
    assert I.boxes_bev(A, C)[0, 0] == 0.0
    S = np.array([[0, 0, 0, 2, 2, 1, 0.0]])                                            # square vs itself turned by 45 deg:
    T = np.array([[0, 0, 0, 2, 2, 1, np.pi / 4]])                                      # regular octagon, area 8(sqrt2-1)
    assert abs(I.boxes_bev(S, T, iou=False)[0, 0] - 8 * (np.sqrt(2) - 1)) < 1e-12
    small = np.array([[0.3, -0.2, 0, 1, 0.5, 1, 1.1]])                                 # contained
    assert abs(I.boxes_bev(A, small, iou=False)[0, 0] - 0.5) < 1e-12
    touch = np.array([[4, 0, 0, 4, 2, 1.5, 0.0]])                                      # sharing an edge: no area
    assert I.boxes_bev(A, touch, iou=False)[0, 0] < 1e-12
    # 3-D IoU: same footprint, half the height overlapping
    U = np.array([[0, 0, 0.75, 4, 2, 1.5, 0.0]])
    assert abs(I.boxes_iou3d(A, U)[0, 0] - (8 * 0.75) / (12 + 12 - 6)) < 1e-12
    # the evaluator's criteria and its clockwise angle: a box and its mirror image overlap like the plain pair
    q = np.array([[0.5, 0.2, 3.0, 1.0, 0.4]])
    r = np.array([[0.0, 0.0, 2.0, 2.0, -0.2]])
    ov = I.rotate_iou_eval(q, r, criterion=2)[0, 0]
    assert abs(I.rotate_iou_eval(q, r, -1)[0, 0] - ov / (3 + 4 - ov)) < 1e-12
    assert abs(I.rotate_iou_eval(q, r, 0)[0, 0] - ov / 3) < 1e-12 and abs(I.rotate_iou_eval(q, r, 1)[0, 0] - ov / 4) < 1e-12
    q7 = np.array([[0.5, 0.2, 0, 3.0, 1.0, 1, -0.4]])
    r7 = np.array([[0.0, 0.0, 0, 2.0, 2.0, 1, 0.2]])
    assert abs(I.boxes_bev(q7, r7, iou=False)[0, 0] - ov) < 1e-12


def _inside(b, X, Y):
    c, s = np.cos(b[6]), np.sin(b[6])
    u = (X - b[0]) * c + (Y - b[1]) * s
    v = -(X - b[0]) * s + (Y - b[1]) * c
    return (np.abs(u) <= b[3] / 2) & (np.abs(v) <= b[4] / 2)


def test_random_pairs_against_a_fine_grid_and_invariances():
    rng = np.random.default_rng(3)
    n = 40
    a = np.zeros((n, 7))
    b = np.zeros((n, 7))
    a[:, :2] = rng.uniform(-3, 3, (n, 2)); b[:, :2] = a[:, :2] + rng.uniform(-2.5, 2.5, (n, 2))
    a[:, 3:5] = rng.uniform(0.8, 5, (n, 2)); b[:, 3:5] = rng.uniform(0.8, 5, (n, 2))
    a[:, 5] = b[:, 5] = 1.5
    a[:, 6] = rng.uniform(-3.2, 3.2, n); b[:, 6] = rng.uniform(-3.2, 3.2, n)
    ov = np.diag(I.boxes_bev(a, b, iou=False))
    # symmetric, invariant under a common rigid motion and under heading + pi
    assert np.allclose(ov, np.diag(I.boxes_bev(b, a, iou=False)), atol=1e-12)
    a2, b2 = a.copy(), b.copy()
    th = 0.83
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    a2[:, :2] = a[:, :2] @ R.T + [7.0, -3.0]; b2[:, :2] = b[:, :2] @ R.T + [7.0, -3.0]
    a2[:, 6] += th; b2[:, 6] += th + np.pi
    assert np.allclose(ov, np.diag(I.boxes_bev(a2, b2, iou=False)), atol=1e-10)
    # brute force: count grid cells inside both rectangles
    g = np.linspace(-9, 9, 1801)
    X, Y = np.meshgrid(g, g)
    cell = (g[1] - g[0]) ** 2
    for i in range(n):
        est = (_inside(a[i], X, Y) & _inside(b[i], X, Y)).sum() * cell
        assert abs(est - ov[i]) < 0.03 + 0.01 * ov[i], (i, est, ov[i])
    assert (ov > 0.5).sum() > 10


def test_nms_is_greedy_on_sorted_scores():
    rng = np.random.default_rng(4)
    n = 200
    boxes = np.zeros((n, 7))
    boxes[:, :2] = rng.uniform(-10, 10, (n, 2))
    boxes[:, 3:6] = rng.uniform(1.5, 4.5, (n, 3))
    boxes[:, 6] = rng.uniform(-3, 3, n)
    scores = rng.permutation(n).astype(np.float64)
    keep, _ = I.nms(boxes, scores, 0.1)
    iou = I.boxes_bev(boxes, boxes)
    order = np.argsort(-scores)
    kept, rem = [], set()
    for i in order:
        if i in rem:
            continue
        kept.append(i)
        for j in order:
            if scores[j] < scores[i] and iou[i, j] > 0.1:
                rem.add(j)
    assert keep.tolist() == kept and 10 < len(kept) < n
    k50, _ = I.nms(boxes, scores, 0.1, pre_maxsize=50)
    assert set(k50.tolist()) <= set(order[:50].tolist()) and len(k50) > 0
    kn, _ = I.nms(boxes, scores, 0.1, normal=True)
    assert 0 < len(kn) <= n


def test_reference_margin_semantics_how_often_a_suppression_decision_differs():
    """The product (and oracle.boxes_bev) return the exact area of the intersection polygon; the reference's kernel
    builds its polygon with a 1e-2 m margin around either box (iou3d_nms_kernel.cu:49-59), restated in
    oracle.overlap_reference_margin.  On 4096 random vehicle-sized boxes of a crowded scene: the difference of the two
    IoU values stays below 2e-2, and the greedy NMS keep lists (scores descending, threshold 0.1 / 0.5 / 0.7) differ in a
    handful of boxes -- the number INTEGRATION.md quotes next to the drop-in claim."""
    rng = np.random.default_rng(2024)
    n = 4096
    boxes = np.zeros((n, 7))
    boxes[:, 0:2] = rng.uniform(-60, 60, (n, 2))
    boxes[:, 2] = rng.uniform(-1.5, -0.5, n)
    boxes[:, 3] = rng.uniform(3.5, 5.5, n); boxes[:, 4] = rng.uniform(1.6, 2.2, n); boxes[:, 5] = rng.uniform(1.4, 1.9, n)
    boxes[:, 6] = rng.uniform(-np.pi, np.pi, n)
    scores = rng.random(n)
    order = np.argsort(-scores, kind="stable")
    B = boxes[order]
    exact = I.boxes_bev(B, B, iou=True)
    iu, ju = np.nonzero(np.triu(exact > 0, 1))
    assert len(iu) > 5000
    # the reference's value for every overlapping pair (a pair that does not overlap exactly can only gain a sliver:
    # pairs closer than the margin are included through the exact IoU of slightly inflated boxes)
    infl = B.copy(); infl[:, 3:5] += 0.03
    ii, jj = np.nonzero(np.triu(I.boxes_bev(infl, infl, iou=True) > 0, 1))
    ref = {}
    worst = 0.0
    for i, j in zip(ii.tolist(), jj.tolist()):
        r = I.iou_bev_reference_margin(B[i], B[j])
        ref[(i, j)] = r
        worst = max(worst, abs(r - exact[i, j]))
    assert worst < 2e-2, worst
    report = {}
    for thr in (0.1, 0.5, 0.7):
        keep_e, keep_r = [], []
        for mode, keep in (("exact", keep_e), ("ref", keep_r)):
            alive = np.ones(n, bool)
            for i in range(n):
                if not alive[i]:
                    continue
                keep.append(i)
                js = np.nonzero(alive & (np.arange(n) > i))[0]
                if mode == "exact":
                    alive[js[exact[i, js] > thr]] = False
                else:
                    for j in js.tolist():
                        if ref.get((i, j), 0.0) > thr:
                            alive[j] = False
        flips = len(set(keep_e) ^ set(keep_r))
        pair_flips = sum(1 for (i, j), r in ref.items() if (r > thr) != (exact[i, j] > thr))
        report[thr] = (len(keep_e), flips, pair_flips)
        assert flips <= 0.01 * n, (thr, flips)
    print("reference-margin vs exact overlap: worst |dIoU| %.4f over %d pairs; (kept, keep-list flips, pair flips) per threshold: %s"
          % (worst, len(ref), report))


def test_a_box_without_area_overlaps_nothing():
    """A point or a segment as the CLIPPING box: its zero-length edges give no half-plane, the result is still 0."""
    A = np.array([[0, 0, 0, 4, 2, 1.5, 0.3]])
    for dx, dy in ((0, 0), (0, 1), (1, 0)):
        Z = np.array([[0.1, 0.1, 0, dx, dy, 1.5, 0.7]])
        assert I.boxes_bev(A, Z, iou=False)[0, 0] == 0.0 and I.boxes_bev(Z, A, iou=False)[0, 0] == 0.0
        assert I.boxes_bev(A, Z)[0, 0] == 0.0 and I.boxes_bev(Z, Z)[0, 0] == 0.0


def test_sparse_nms_is_the_dense_one():
    """`nms_sparse` / `pair_ious` (no n x n matrix) against the dense `nms`: the same keep list and, pair by pair, the
    same float64 IoU; every pair the sparse list leaves out is exactly 0 in the dense matrix."""
    from tests import iou3d_cases as C
    for n, thresh, pre, normal in ((2000, 0.2, None, False), (2100, 0.3, 1500, False), (1900, 0.25, None, True),
                                   (1, 0.1, None, False), (2, 0.1, 5, True)):
        boxes = C.random_boxes(np.random.default_rng(n), n, 4.0 * n ** 0.25 + 4.0)
        scores = np.random.default_rng(n + 1).permutation(n).astype(np.float32)
        keep_d, iou_d = I.nms(boxes, scores, thresh, pre_maxsize=pre, normal=normal)
        keep_s, (i, j, iou_s) = I.nms_sparse(boxes, scores, thresh, pre_maxsize=pre, normal=normal)
        assert np.array_equal(keep_d, keep_s) and keep_s.dtype == keep_d.dtype
        assert (j > i).all() and np.array_equal(iou_s, iou_d[i, j])
        assert (np.diff(i) >= 0).all() and ((np.diff(i) > 0) | (np.diff(j) > 0)).all()      # sorted, no pair twice
        rest = np.triu(iou_d, 1)
        rest[i, j] = 0.0
        assert not rest.any()
        if n >= 1900:
            assert 0.2 * len(iou_d) < len(keep_d) < 0.8 * len(iou_d) and (iou_s > thresh).sum() > 500
            # a second threshold walked over the same pair list
            keep_2, _ = I.nms_sparse(boxes, scores, 0.5, pre_maxsize=pre, normal=normal, pairs=(i, j, iou_s))
            assert np.array_equal(keep_2, I.nms(boxes, scores, 0.5, pre_maxsize=pre, normal=normal, iou=iou_d)[0])


def test_widest_gap_threshold():
    thr, half = I.widest_gap_threshold([0.1, 0.195, 0.197, 0.204, 0.2045, 0.3], 0.2)
    assert abs(thr - 0.2005) < 1e-12 and abs(half - 0.0035) < 1e-12
    thr, half = I.widest_gap_threshold([], 0.2)                      # nothing in the window: its two ends bound the gap
    assert abs(thr - 0.2) < 1e-12 and abs(half - 0.01) < 1e-12
    thr, half = I.widest_gap_threshold([0.2], 0.2)                   # never ON a value
    assert abs(abs(thr - 0.2) - 0.005) < 1e-12 and abs(half - 0.005) < 1e-12


def test_the_gpu_nms_cases_have_no_pair_near_their_threshold():
    """What tests/test_gpu_iou3d.py relies on, on the oracle alone: every case's threshold sits in a gap whose
    half-width exceeds the 1e-5 the GPU IoU is asserted to, and the cases with more than 4096 boxes suppress a real
    share.  (The 4 m x 4 m case of 2500 boxes is asserted in the GPU test only: it has 3e6 overlapping pairs.)"""
    from tests import iou3d_cases as C
    seen = {}
    for n, nominal, pre, normal in C.NMS_CASES:
        boxes, scores = C.nms_scene(n)
        order = np.argsort(-scores.astype(np.float64), kind="stable")[:pre]
        pairs = I.pair_ious(boxes[order], normal=normal)
        thr, half = I.widest_gap_threshold(pairs[2], nominal)
        assert half > 1e-5 and abs(thr - nominal) < 0.01, (n, thr, half)
        assert not (np.abs(pairs[2] - thr) < half * (1 - 1e-9)).any()
        keep, _ = I.nms_sparse(boxes, scores, thr, pre, normal, pairs=pairs)
        seen[(n, nominal, pre, normal)] = (round(thr, 6), half, len(keep))
        if n > 4096:
            assert 0.2 * len(order) < len(keep) < 0.8 * len(order), (n, len(keep))
    print("NMS cases (threshold, half-width of its gap, kept):", seen)
    assert seen[(4096, 0.2, 3000, False)][0] == 0.20584
