"""The overlap kernels of row f-3 (csrc/iou_stage.hip, csrc/rect_overlap.hpp) on the inputs where polygon clippers go
wrong, against the float64 world-frame checker (oracle/iou3d_oracle.py): degenerate pairs (tests/iou3d_cases.py) in one
matrix call with ordinary pairs around them, both roles (the kernel clips A in B's frame), under a rigid motion, at
the tile edges of k_pair_matrix (8 x 32) and k_pair_list (256), at the grid limit, and through the evaluator's
(cx, cy, w, h, angle) entry.  Tolerances are the ones tests/test_gpu_iou3d.py states: IoU 1e-5 absolute near the origin,
overlap rtol 1e-5 / atol 1e-4, and coordinate magnitude x 2^-24 x perimeter in play on top where boxes are far out."""
import numpy as np
import pytest
import torch

from oracle import iou3d_oracle as I
from tests import iou3d_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _gpu(a, b, iou):
    from dfu3d_amd import stages as st
    return st.boxes_bev(torch.from_numpy(np.ascontiguousarray(a)).to(DEV), torch.from_numpy(np.ascontiguousarray(b)).to(DEV),
                        iou=iou).cpu().numpy()


def _mixed_scene(seed):
    """The families' rows and columns shuffled among ordinary random boxes: every 8 x 32 tile of the matrix holds pairs of
    both kinds, so a vertex written into a neighbour's LDS column would damage an ordinary entry."""
    rng = np.random.default_rng(seed)
    A, B, blocks = C.family_blocks(rng, groups=4)
    A = np.concatenate([A, C.random_boxes(rng, 3 * len(A), 8.0)])
    B = np.concatenate([B, C.random_boxes(rng, 3 * len(B), 8.0)])
    pa, pb = rng.permutation(len(A)), rng.permutation(len(B))
    where_a, where_b = np.argsort(pa), np.argsort(pb)
    blocks = {k: [(where_a[r], where_b[c]) for r, c in v] for k, v in blocks.items()}
    return A[pa], B[pb], blocks


def _check_matrix(a, b, extra_atol=0.0):
    """GPU overlap / IoU matrices of (a, b) against the checker, and the role swap.  extra_atol: (n, m) array."""
    exp_ov, exp_iou = I.boxes_bev(a, b, iou=False), I.boxes_bev(a, b)
    ov, iou = _gpu(a, b, False), _gpu(a, b, True)
    ov_t, iou_t = _gpu(b, a, False).T, _gpu(b, a, True).T
    for m in (ov, iou, ov_t, iou_t):
        assert m.dtype == np.float32 and m.shape == exp_ov.shape and np.isfinite(m).all()
    tol_ov = 1e-4 + 1e-5 * exp_ov + extra_atol
    err = np.abs(ov - exp_ov)
    print("  overlap: worst error / tolerance %.3g (error %.3g); IoU: worst error %.3g; role swap: %.3g"
          % ((err / tol_ov).max(), err.max(), np.abs(iou - exp_iou).max(), np.abs(ov - ov_t).max()))
    assert (err <= tol_ov).all(), np.unravel_index((err / tol_ov).argmax(), err.shape)
    assert (np.abs(ov_t - exp_ov) <= tol_ov).all()
    assert (np.abs(ov - ov_t) <= tol_ov).all()                         # A clipped in B's frame against B clipped in A's
    if np.ndim(extra_atol) == 0 and extra_atol == 0.0:
        np.testing.assert_allclose(iou, exp_iou, rtol=0, atol=1e-5)
        np.testing.assert_allclose(iou_t, exp_iou, rtol=0, atol=1e-5)
    assert (iou >= 0).all() and (iou <= 1 + 1e-5).all() and (iou_t >= 0).all() and (iou_t <= 1 + 1e-5).all()
    assert (ov >= 0).all() and (ov_t >= 0).all()
    return ov, iou, exp_ov, exp_iou


def test_degenerate_families_among_ordinary_pairs_in_one_matrix():
    a, b, blocks = _mixed_scene(41)
    assert len(a) > 1000 and len(b) > 1000
    ov, iou, exp_ov, exp_iou = _check_matrix(a, b)
    for name, bl in blocks.items():                                    # a few hundred pairs of each family were in it
        pairs = sum(len(r) * len(c) for r, c in bl)
        assert pairs >= 100, (name, pairs)
    r, c = blocks["identical"][0]
    assert np.abs(iou[np.ix_(r, c)] - 1.0).max() < 1e-5
    for r, c in blocks["cross"]:                                       # the last two pairs: unit squares at 45 degrees
        assert np.abs(ov[r[-1], c[-2:]] - 8 * (np.sqrt(2) - 1) / 4).max() < 1e-4
    for name in ("zero_a", "zero_b", "zero_both", "shared_edge"):
        for r, c in blocks[name]:
            assert exp_ov[np.ix_(r, c)].max() < 1e-5 and ov[np.ix_(r, c)].max() < 1.2e-4       # no area in common


@pytest.mark.parametrize("shift", [(70.0, 40.0), (-70.0, 40.0), (70.0, -40.0), (-70.0, -40.0)])
def test_degenerate_families_under_a_rigid_motion(shift):
    """The same pairs moved by (+-70, +-40) m and turned by a common angle.  On top of the near-origin tolerance: largest
    coordinate of the pair x 2^-24 (float32 resolution of the inputs the kernel subtracts) x the perimeter in play (the
    overlap polygon lies in both boxes, so the smaller of the two perimeters bounds it)."""
    a, b, _ = _mixed_scene(43)
    turn = {(70.0, 40.0): 0.37, (-70.0, 40.0): np.pi / 2, (70.0, -40.0): -2.2, (-70.0, -40.0): 3.0}[shift]
    a, b = C.rigid_motion(a, shift, turn), C.rigid_motion(b, shift, turn)
    reach = lambda x: np.abs(x[:, :2]).max(1).astype(np.float64) + 0.5 * np.hypot(x[:, 3], x[:, 4])
    perim = lambda x: 2.0 * (x[:, 3].astype(np.float64) + x[:, 4])
    extra = np.maximum(reach(a)[:, None], reach(b)[None, :]) * 2.0 ** -24 * np.minimum(perim(a)[:, None], perim(b)[None, :])
    _check_matrix(a, b, extra_atol=extra)


def test_tile_edges_of_the_matrix_kernel():
    rng = np.random.default_rng(47)
    shapes = [(n, m) for n in (1, 7, 8, 9) for m in (1, 31, 32, 33, 64, 65)] + [(1, 5000), (5000, 1)]
    for n, m in shapes:
        a, b = C.random_boxes(rng, n, 4.0), C.random_boxes(rng, m, 4.0)
        a[-1], b[-1] = a[0], a[0]                                      # the last row / column is never all zero
        ov, iou, exp_ov, exp_iou = _check_matrix(a, b)
        assert ov.shape == (n, m) and abs(iou[-1, -1] - 1.0) < 1e-5 and (exp_ov > 0).mean() > 0.2


def test_grid_limit_of_the_matrix_kernel():
    """(n + 7) / 8 workgroups along y: 65535 of them work, one more is DFU3D_ERANGE."""
    from dfu3d_amd import _lib
    rng = np.random.default_rng(53)
    n = 8 * 65535
    a = C.random_boxes(rng, n + 1, 8.0)
    b = np.array([[0.5, -0.25, 0, 6.0, 5.0, 1.5, 0.4]], np.float32)
    a[n - 1] = b[0]
    ov, iou = _gpu(a[:n], b, False), _gpu(a[:n], b, True)
    assert ov.shape == (n, 1) and np.isfinite(ov).all() and np.isfinite(iou).all() and iou.min() >= 0 and iou.max() <= 1 + 1e-5
    rows = np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), rng.integers(0, n, 4000)]))
    exp_ov, exp_iou = I.boxes_bev(a[rows], b, iou=False), I.boxes_bev(a[rows], b)
    np.testing.assert_allclose(ov[rows], exp_ov, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(iou[rows], exp_iou, rtol=0, atol=1e-5)
    assert abs(iou[n - 1, 0] - 1.0) < 1e-5 and (exp_ov > 0).sum() > 1000
    with pytest.raises(_lib.Dfu3dError, match=r"\(-3\)"):
        _gpu(a, b, True)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_paired_entry_point(n):
    """dfu3d_boxes_bev_paired (k_pair_list, 256 pairs per workgroup) directly: against the checker's diagonal and
    against the diagonal of the GPU matrix call."""
    from dfu3d_amd import stages as st
    rng = np.random.default_rng(59 + n)
    fa, fb, _, _ = C.family_pairs(rng, groups=1)
    pick = rng.permutation(len(fa))[:n // 2]
    a = np.concatenate([fa[pick], C.random_boxes(rng, n - len(pick), 3.0)])
    b = np.concatenate([fb[pick], C.random_boxes(rng, n - len(pick), 3.0)])
    perm = rng.permutation(n)
    a, b = a[perm], b[perm]
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    exp_ov = I._clip_pairs(I._corners7(a), I._corners7(b))
    area = lambda x: x[:, 3].astype(np.float64) * x[:, 4]
    exp_iou = exp_ov / np.maximum(area(a) + area(b) - exp_ov, 1e-8)
    ov, iou = st.boxes_bev_paired(ta, tb, iou=False).cpu().numpy(), st.boxes_bev_paired(ta, tb, iou=True).cpu().numpy()
    assert ov.shape == (n,) and iou.shape == (n,) and np.isfinite(ov).all() and np.isfinite(iou).all()
    np.testing.assert_allclose(ov, exp_ov, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(iou, exp_iou, rtol=0, atol=1e-5)
    np.testing.assert_allclose(ov, np.diag(st.boxes_bev(ta, tb, iou=False).cpu().numpy()), rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(iou, np.diag(st.boxes_bev(ta, tb, iou=True).cpu().numpy()), rtol=0, atol=1e-5)
    assert iou.min() >= 0 and iou.max() <= 1 + 1e-5 and (n < 255 or (exp_ov > 0).sum() > n // 4)
    # the other way round: the overlap is symmetric
    np.testing.assert_allclose(st.boxes_bev_paired(tb, ta, iou=False).cpu().numpy(), exp_ov, rtol=1e-5, atol=1e-4)


@pytest.mark.parametrize("criterion", [-1, 0, 1, 2])
def test_degenerate_families_through_the_evaluator_entry(criterion):
    """rotate_iou_gpu_eval on the same footprints as (cx, cy, w, h, angle).  Criteria 0 and 1 divide the overlap by ONE
    box's area (floor 1e-8, as in the reference), which multiplies the overlap's float32 error by 1 / area.  The
    tolerance of test_rotate_iou_eval_mirror was stated for ordinary boxes (sides from 0.5 m); it is kept for every
    entry whose denominator is at least 0.25 m^2.  Below that (slivers, 5 cm boxes, boxes without area) the quotient is
    multiplied back by its denominator and held to the overlap tolerance (rtol 1e-5, atol 1e-4)."""
    from dfu3d_amd.pcdet_kitti.rotate_iou import rotate_iou_gpu_eval
    a7, b7, _ = _mixed_scene(61)
    q, r = C.to_fmt5(a7[:700]), C.to_fmt5(b7[:900])
    got = rotate_iou_gpu_eval(q, r, criterion)
    exp = I.rotate_iou_eval(q, r, criterion)
    assert got.dtype == np.float32 and got.shape == exp.shape and np.isfinite(got).all() and (got >= 0).all()
    den = np.ones(exp.shape)
    if criterion == 0:
        den = den * np.maximum(q[:, 2].astype(np.float64) * q[:, 3], 1e-8)[:, None]
    if criterion == 1:
        den = den * np.maximum(r[:, 2].astype(np.float64) * r[:, 3], 1e-8)[None, :]
    small = den < 0.25
    assert criterion in (0, 1) or not small.any()
    atol = 1e-5 if criterion != 2 else 1e-4
    err = np.abs(got - exp)
    print("  criterion %d: worst error %.3g on ordinary denominators, %.3g on the overlap of %d small ones"
          % (criterion, err[~small].max(), (err * den)[small].max() if small.any() else 0.0, small.sum()))
    assert (err[~small] <= atol + 1e-5 * exp[~small]).all(), err[~small].max()
    assert ((err * den)[small] <= 1e-4 + 1e-5 * (exp * den)[small]).all()
    if criterion == -1:
        assert got.max() <= 1 + 1e-5
        np.testing.assert_allclose(got, I.boxes_bev(a7[:700], b7[:900]), rtol=0, atol=1e-5)    # the same footprints as fmt 7


def test_the_evaluator_angle_turns_clockwise():
    """One readable pair: a 4 x 1 box turned by +0.6 about the origin and a level 4 x 1 box below and to the right of
    it.  Clockwise (rotate_iou.py's corner formula) the first box points down towards the second; counter-clockwise it
    points away."""
    from dfu3d_amd.pcdet_kitti.rotate_iou import rotate_iou_gpu_eval
    q = np.array([[0.0, 0.0, 4.0, 1.0, 0.6]], np.float32)
    r = np.array([[1.2, -0.8, 4.0, 1.0, 0.0]], np.float32)
    cw = I.rotate_iou_eval(q, r, 2)[0, 0]
    ccw = I.rotate_iou_eval(q * np.array([1, 1, 1, 1, -1], np.float32), r, 2)[0, 0]
    assert cw > 0.5 and abs(cw - ccw) > 0.1 * max(cw, ccw), (cw, ccw)
    got = rotate_iou_gpu_eval(q, r, 2)[0, 0]
    assert abs(got - cw) <= 1e-4 + 1e-5 * cw, (got, cw, ccw)
