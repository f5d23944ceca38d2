"""A sequential NumPy restatement of THE RULE and THE SHUFFLE of csrc/dfu3d_smp.h (DataProcessor.sample_points for a
batch), taking the same three blocks of random words as the stage, and the contract every output of the reference's
sample_points keeps whatever its random draws were."""
import numpy as np

NEAR = np.float32(40.0)


def depth(xyz):
    """fl32(sqrt(fl32(fl32(x*x + y*y) + z*z))), every operation rounded to float32 on its own."""
    x, y, z = (np.asarray(xyz[:, k], np.float32) for k in range(3))
    with np.errstate(all="ignore"):
        return np.sqrt(((x * x).astype(np.float32) + (y * y).astype(np.float32)).astype(np.float32)
                       + (z * z).astype(np.float32), dtype=np.float32)


def near_flags(xyz):
    with np.errstate(all="ignore"):
        return depth(xyz) < NEAR                                 # a NaN depth is not near


def _smallest(sel, rows, m):
    """The m rows of `rows` (ascending) smallest by (sel[row], row), in ascending row order."""
    rows = np.asarray(rows, np.int64)
    pick = sorted(rows.tolist(), key=lambda r: (int(sel[r]), r))[:m]
    return sorted(pick)


def chosen_list(xyz, K, sel, rep):
    """xyz float32 (n, >= 3) of one scene; sel uint32 (n); rep uint32 (K) -> the list L: K scene-local rows (n == 0: none)."""
    n = len(xyz)
    sel, rep = np.asarray(sel).view(np.uint32), np.asarray(rep).view(np.uint32)
    if n == 0:
        return []
    if n > K:
        near = near_flags(xyz)
        far = np.flatnonzero(~near)
        if len(far) < K:
            return sorted(far.tolist() + _smallest(sel, np.flatnonzero(near), K - len(far)))
        return _smallest(sel, np.arange(n), K)
    L = list(range(n))
    if K == n:
        return L
    if K - n <= n:
        return L + _smallest(sel, np.arange(n), K - n)
    return L + [(int(rep[j]) * n) >> 32 for j in range(K - n)]


def shuffle_slots(ord_row):
    """The slots 0 .. K-1 ascending by (ord[j], j)."""
    return np.argsort(np.asarray(ord_row).view(np.uint32), kind="stable")


def sample_rows(xyz, K, sel, ord_row, rep):
    """One scene -> the K scene-local rows of its output, in output order (empty scene: K times -1)."""
    L = chosen_list(xyz, K, sel, rep)
    if not L:
        return np.full(K, -1, np.int64)
    return np.asarray(L, np.int64)[shuffle_slots(ord_row)]


def sample_points_ref(points, point_cnt, K, out_cols, sel, ord_, rep):
    """points float32 (R, 1 + C); point_cnt (B); sel (R), ord_, rep (B, K) int32 or uint32 -> (out float32 (B * K,
    1 + out_cols), status word, rows int64 (B, K) scene-local)."""
    points = np.asarray(points, np.float32)
    B = len(point_cnt)
    out = np.zeros((B * K, 1 + out_cols), np.float32)
    rows = np.zeros((B, K), np.int64)
    status, start = 0, 0
    sel = np.asarray(sel).view(np.uint32)
    for b in range(B):
        n = int(point_cnt[b])
        scene = points[start:start + n]
        r = sample_rows(scene[:, 1:4], K, sel[start:start + n], np.asarray(ord_)[b], np.asarray(rep)[b])
        rows[b] = r
        out[b * K:(b + 1) * K, 0] = b
        if n == 0:
            status |= 1
        else:
            out[b * K:(b + 1) * K, 1:] = scene[r, 1:1 + out_cols]
        start += n
    return out, status, rows


def check_contract(points, rows_out, K):
    """points (n, >= 3) of one scene (xyz first); rows_out: the scene-local rows of a sampled cloud, in any order.
    Asserts what sample_points promises for every draw."""
    n = len(points)
    rows_out = np.asarray(rows_out, np.int64)
    assert rows_out.shape == (K,), (rows_out.shape, K)
    assert n > 0 and rows_out.min() >= 0 and rows_out.max() < n
    count = np.bincount(rows_out, minlength=n)
    if n > K:
        far = ~near_flags(np.asarray(points, np.float32)[:, 0:3])
        assert count.max() == 1, "a row twice"
        if far.sum() < K:
            assert (count[far] == 1).all(), "a far row is missing"
    elif K <= 2 * n:
        assert count.min() >= 1 and count.max() <= 2, "every row once or twice"
    else:
        assert count.min() >= 1, "every row at least once"


def check_frequencies(rows, n, sigmas=5.0):
    """rows (B, K): the scene-local rows of B independent draws of K out of n rows without replacement (all near).
    Every row's inclusion count within `sigmas` binomial standard deviations of B * K / n, and its mean output slot
    within `sigmas` standard deviations of the mean of a uniform slot, (K - 1) / 2 (variance (K * K - 1) / 12 per draw)."""
    rows = np.asarray(rows, np.int64)
    B, K = rows.shape
    q = K / n
    count = np.bincount(rows.ravel(), minlength=n)
    assert len(count) == n and count.sum() == B * K
    dev = np.abs(count - B * q) / np.sqrt(B * q * (1 - q))
    assert dev.max() <= sigmas, ("inclusion", int(dev.argmax()), float(dev.max()))
    slot_sum = np.bincount(rows.ravel(), weights=np.tile(np.arange(K), B).astype(np.float64), minlength=n)
    sd = np.sqrt((K * K - 1) / 12.0 / count)
    dev = np.abs(slot_sum / count - (K - 1) / 2.0) / sd
    assert dev.max() <= sigmas, ("slot", int(dev.argmax()), float(dev.max()))
