"""The oracle of the batched proposal stage (csrc/proposal_stage.hip), with no kernel of that file in it.

order_ref      THE ORDER RULE of csrc/dfu3d_prop.h in NumPy, exact: the monotone uint32 key of the float32 score (-0.0 as
               +0.0, every NaN the one key above +inf), equal keys by ascending point index.
walk_ref       per sample the point indices of ALL survivors, best first: the existing NMS kernel (stages.nms_bev) on the
               boxes already put in order_ref's order -- it sorts nothing itself, and decides every pair with the same
               nms_suppresses as the kernels under test.  Needs the GPU.
pad_ref        the padded outputs for a post_max from walk_ref's lists: the first post_max survivors of the full greedy walk
               are the survivors of the walk stopped at post_max, so truncating on the host is the whole specification.
proposals_ref  the three together.

Case generators for the tests sit below."""
import numpy as np

f32 = np.float32
NAN_KEY = np.uint32(0xFFFFFFFF)


def sort_key(scores):
    """float32 scores -> uint32 keys, larger = better."""
    s = np.ascontiguousarray(scores, f32)
    u = s.view(np.uint32).copy()
    u[u == np.uint32(0x80000000)] = 0                                    # -0.0 is +0.0
    neg = (u & np.uint32(0x80000000)) != 0
    key = np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)
    key[np.isnan(s)] = NAN_KEY
    return key


def order_ref(scores, pre_max):
    """scores float32 (N) -> int64 (min(pre_max, N)): the best points, best first."""
    key = sort_key(scores).astype(np.int64)
    idx = np.arange(key.shape[0], dtype=np.int64)
    return idx[np.lexsort((idx, -key))][:max(int(pre_max), 0)]


def walk_ref(scores, boxes, thresh, pre_max, device="cuda:0"):
    """scores (B, N), boxes (B, N, C) -> [int64 point indices of every survivor of sample b, best first]."""
    import torch
    from dfu3d_amd import stages
    out = []
    for b in range(scores.shape[0]):
        order = order_ref(scores[b], pre_max)
        if order.size == 0:
            out.append(order)
            continue
        rows = torch.from_numpy(np.ascontiguousarray(boxes[b][order][:, :7], f32)).to(device).contiguous()
        keep, n = stages.nms_bev(rows, float(thresh))
        out.append(order[keep[:n].cpu().numpy()])
    return out


def pad_ref(kept, scores, labels, boxes, post_max):
    B, _, C = boxes.shape
    rois = np.zeros((B, post_max, C), f32)
    roi_scores = np.zeros((B, post_max), f32)
    roi_labels = np.ones((B, post_max), np.int64)
    roi_point_idx = np.full((B, post_max), -1, np.int64)
    num_rois = np.zeros((B,), np.int32)
    for b, k in enumerate(kept):
        k = k[:post_max]
        n = len(k)
        rois[b, :n], roi_scores[b, :n], roi_labels[b, :n], roi_point_idx[b, :n] = boxes[b][k], scores[b][k], labels[b][k] + 1, k
        num_rois[b] = n
    return rois, roi_scores, roi_labels, roi_point_idx, num_rois


def proposals_ref(scores, labels, boxes, thresh, pre_max, post_max, device="cuda:0"):
    return pad_ref(walk_ref(scores, boxes, thresh, pre_max, device), scores, labels, boxes, post_max)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ---- generators --------------------------------------------------------------------------------------------------------
def distinct_scores(rng, B, N, lo=-3.0, hi=3.0):
    """(B, N) float32: every row a random permutation of N distinct values."""
    base = np.linspace(lo, hi, N).astype(f32) if N > 1 else np.array([0.25], f32)
    assert len(np.unique(base)) == N
    return np.stack([rng.permutation(base) for _ in range(B)])


def clustered_boxes(rng, B, N, C=7, centres=6, jitter=0.4, spread=30.0, scattered=0.0):
    """(B, N, C) float32: car-sized boxes drawn around `centres` places per sample (centre, size and heading jittered), so
    that suppression is common; a fraction `scattered` of them anywhere in the field.  Columns beyond 6 are random."""
    out = np.zeros((B, N, C), f32)
    for b in range(B):
        c = rng.uniform(-spread, spread, (centres, 2))
        h = rng.uniform(-np.pi, np.pi, centres)
        which = rng.integers(0, centres, N)
        out[b, :, 0:2] = c[which] + rng.normal(0, jitter, (N, 2))
        out[b, :, 2] = rng.normal(-1.0, 0.2, N)
        out[b, :, 3:6] = np.array([3.9, 1.6, 1.56]) * (1 + rng.normal(0, 0.25 * jitter, (N, 3)).clip(-0.5, 0.5))
        out[b, :, 6] = h[which] + rng.normal(0, 0.5 * jitter, N)
        loose = rng.uniform(0, 1, N) < scattered
        out[b, loose, 0:2] = rng.uniform(-spread, spread, (int(loose.sum()), 2))
        out[b, loose, 6] = rng.uniform(-np.pi, np.pi, int(loose.sum()))
        if C > 7:
            out[b, :, 7:] = rng.normal(0, 1, (N, C - 7))
    return out


def site(k):
    """Centres of disjoint 8 m cells."""
    k = np.asarray(k)
    return 8.0 + 8.0 * (k % 64), 8.0 + 8.0 * (k // 64)


def disjoint_boxes(n, C=7):
    """2 x 1 boxes, heading 0, one per cell: no two overlap.  Power-of-two coordinates: every area and IoU is exact."""
    b = np.zeros((n, C), f32)
    b[:, 0], b[:, 1] = site(np.arange(n))
    b[:, 3], b[:, 4], b[:, 5] = 2.0, 1.0, 1.0
    return b


def by_position(rng, rows):
    """rows (n, C) in the walk's order -> (scores (1, n), boxes (1, n, C), perm): row p sits at point perm[p], and the
    scores, distinct, fall with p -- so the order stage has to undo the permutation."""
    n = rows.shape[0]
    perm = rng.permutation(n)
    scores = np.zeros((1, n), f32)
    scores[0, perm] = np.linspace(2.0, -2.0, n).astype(f32) if n > 1 else f32(0.5)
    boxes = np.zeros((1,) + rows.shape, f32)
    boxes[0, perm] = rows
    return scores, boxes, perm
