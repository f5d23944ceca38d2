"""f-3 on the GPU against the independent float64 checker (oracle/iou3d_oracle.py: world-frame polygon
clipping, no code or formulation shared with the kernels): overlap / IoU within 1e-5 absolute, NMS keep lists identical
at thresholds that no pair of the scene is near (tests/iou3d_cases.py).  Clipper edge cases: tests/test_gpu_iou3d_edges.py;
NMS patterns with answers known in closed form: tests/test_gpu_nms_patterns.py."""
import numpy as np
import pytest
import torch

from oracle import iou3d_oracle as I
from tests import iou3d_cases as C

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


_boxes = C.random_boxes


def test_bev_overlap_iou_and_volume_iou_match_the_checker():
    from dfu3d_amd.pcdet_kitti import iou3d_nms_utils as U
    from dfu3d_amd import stages as st
    rng = np.random.default_rng(21)
    for n, m in ((0, 4), (1, 1), (17, 33), (130, 257)):
        a, b = _boxes(rng, max(n, 1), 8.0)[:n], _boxes(rng, m, 8.0)
        if n and m:
            b[0] = a[0]                                     # identical pair
            if m > 1:
                b[1] = a[0]; b[1, 6] += np.float32(np.pi / 2)   # same box turned by 90 degrees
            if m > 2:
                b[2] = a[0]; b[2, 0] += a[0, 3]                 # pushed along x by its own length (heading aside)
        ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
        iou = U.boxes_iou_bev(ta, tb).cpu().numpy()
        ov = st.boxes_bev(ta, tb, iou=False).cpu().numpy()
        exp_iou, exp_ov = I.boxes_bev(a, b), I.boxes_bev(a, b, iou=False)
        assert iou.shape == (n, m)
        np.testing.assert_allclose(iou, exp_iou, rtol=0, atol=1e-5)
        np.testing.assert_allclose(ov, exp_ov, rtol=1e-5, atol=1e-4)
        if n and m:
            assert abs(iou[0, 0] - 1.0) < 1e-5 and (exp_iou > 0).sum() >= min(m, 2)
            i3 = U.boxes_iou3d_gpu(ta, tb).cpu().numpy()
            np.testing.assert_allclose(i3, I.boxes_iou3d(a, b), rtol=0, atol=1e-5)
            k = min(n, m)
            al = U.boxes_aligned_iou3d_gpu(ta[:k], tb[:k]).cpu().numpy()
            assert al.shape == (k, 1)
            np.testing.assert_allclose(al[:, 0], np.diag(I.boxes_iou3d(a[:k], b[:k])), rtol=0, atol=1e-5)


def test_far_from_the_origin_and_degenerate_boxes():
    """Box centres at hundreds of metres (float32 has ~3e-5 m resolution there: the kernels work relative to one box),
    zero-size boxes, and boxes that only touch."""
    from dfu3d_amd import stages as st
    rng = np.random.default_rng(5)
    a = _boxes(rng, 64, 3.0)
    b = _boxes(rng, 64, 3.0)
    a[:, :2] += np.float32(400.0); b[:, :2] += np.float32(400.0)
    b[0] = a[0]
    a[1, 3] = 0.0                                           # degenerate: no area
    b[2] = a[2]; b[2, 0] += a[2, 3] * np.cos(a[2, 6]); b[2, 1] += a[2, 3] * np.sin(a[2, 6])   # touching along an edge
    ov = st.boxes_bev(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), iou=False).cpu().numpy()
    exp = I.boxes_bev(a, b, iou=False)
    np.testing.assert_allclose(ov, exp, rtol=2e-5, atol=2e-3)       # 400 m * 2^-24 * perimeter
    assert (ov[1] < 1e-6).all() and ov[2, 2] < 2e-3            # a zero-width box has no area (up to float32 dust)
    assert np.isfinite(ov).all()


@pytest.mark.parametrize("criterion", [-1, 0, 1, 2])
def test_rotate_iou_eval_mirror(criterion):
    """The AP evaluator's entry point (numba-CUDA in the reference): NumPy in, NumPy float32 out."""
    from dfu3d_amd.pcdet_kitti.rotate_iou import rotate_iou_gpu_eval
    rng = np.random.default_rng(31 + criterion)
    n, k = 77, 130
    q = np.zeros((n, 5), np.float32); r = np.zeros((k, 5), np.float32)
    q[:, :2] = rng.uniform(-12, 12, (n, 2)); r[:, :2] = rng.uniform(-12, 12, (k, 2))
    q[:, 2:4] = rng.uniform(0.5, 5, (n, 2)); r[:, 2:4] = rng.uniform(0.5, 5, (k, 2))
    q[:, 4] = rng.uniform(-3.2, 3.2, n); r[:, 4] = rng.uniform(-3.2, 3.2, k)
    r[:5] = q[:5]
    got = rotate_iou_gpu_eval(q, r, criterion)
    assert got.dtype == np.float32 and got.shape == (n, k)
    exp = I.rotate_iou_eval(q, r, criterion)
    np.testing.assert_allclose(got, exp, rtol=1e-5, atol=1e-5 if criterion != 2 else 1e-4)
    assert (exp > 0).sum() > 50
    assert rotate_iou_gpu_eval(q[:0], r, criterion).shape == (0, k)


def _nms_against_the_checker(n, nominal, pre, normal, spread=None):
    """No pair may be ambiguous, so the keep lists must be EQUAL: the threshold is moved (by less than 0.01) into the
    widest gap between oracle IoU values, the half-width of that gap exceeds the 1e-5 this file asserts for the IoU,
    and (up to 4096 boxes, rotated) the GPU's IoU of every candidate pair is asserted within that 1e-5.  The threshold
    reaches the kernel as a float32; its rounding (1e-8) is inside the margin."""
    from dfu3d_amd.pcdet_kitti import iou3d_nms_utils as U
    from dfu3d_amd import stages as st
    boxes, scores = C.nms_scene(n, spread)
    order = np.argsort(-scores.astype(np.float64), kind="stable")[:pre]
    pairs = I.pair_ious(boxes[order], normal=normal)
    thresh, half = I.widest_gap_threshold(pairs[2], nominal)
    exp, _ = I.nms_sparse(boxes, scores, thresh, pre_maxsize=pre, normal=normal, pairs=pairs)
    print("nms case n=%d pre=%s normal=%s: %d candidate pairs, threshold %.6f, half-width of its gap %.3g, oracle keeps %d"
          % (n, pre, normal, pairs[0].size, thresh, half, len(exp)))
    assert half > 1e-5 and abs(thresh - nominal) < 0.01, (thresh, half)        # on the oracle, before the GPU is touched
    assert not (np.abs(pairs[2] - thresh) <= 1e-5).any()
    if len(order) > 4096 or spread is not None:
        assert 0.2 * len(order) < len(exp) < 0.8 * len(order), (len(exp), len(order))    # a trivial walk cannot pass
    tb, ts = torch.from_numpy(boxes).to(DEV), torch.from_numpy(scores).to(DEV)
    if len(order) <= 4096 and not normal:
        sb = torch.from_numpy(boxes[order]).to(DEV)
        iou = st.boxes_bev(sb, sb, iou=True).cpu().numpy()
        err = np.abs(iou[pairs[0], pairs[1]] - pairs[2])
        print("  GPU IoU of the candidate pairs: worst |error| %.3g" % (err.max() if err.size else 0.0))
        assert (err <= 1e-5).all(), err.max()
    if normal:
        assert pre is None
        sel, _ = U.nms_normal_gpu(tb, ts, thresh)
    else:
        sel, _ = U.nms_gpu(tb, ts, thresh, pre_maxsize=pre)
    got = sel.cpu().numpy()
    assert got.dtype == np.int64 and 0 < len(got) <= n
    assert np.array_equal(got, exp), (n, len(got), len(exp), int((got[:min(len(got), len(exp))] != exp[:min(len(got), len(exp))]).argmax()))


@pytest.mark.parametrize("n,thresh,pre,normal", C.NMS_CASES)
def test_nms_matches_the_checker(n, thresh, pre, normal):
    _nms_against_the_checker(n, thresh, pre, normal)


def test_nms_dense_scene_at_a_high_threshold():
    """2500 boxes on 4 m x 4 m at 0.7: a third is suppressed (the 2500-box case above keeps 99.5 %)."""
    n, nominal, spread = C.DENSE_2500
    _nms_against_the_checker(n, nominal, None, False, spread=spread)


def test_nms_more_boxes_than_the_abi_admits():
    """32769 boxes: DFU3D_ERANGE, as an exception from the wrapper and with `keep` / `num_keep` untouched at the C ABI."""
    import ctypes
    from dfu3d_amd import _lib, stages as st
    n = 32769
    boxes = torch.from_numpy(C.random_boxes(np.random.default_rng(3), n, 200.0)).to(DEV)
    for normal in (False, True):
        with pytest.raises(_lib.Dfu3dError, match=r"\(-3\)"):
            st.nms_bev(boxes, 0.2, normal=normal)
        keep = torch.full((n,), -1, dtype=torch.int64, device=DEV)
        num = torch.full((1,), -7, dtype=torch.int32, device=DEV)
        mask = torch.zeros(64, dtype=torch.int64, device=DEV)         # never touched: the size check comes first
        fn = _lib.lib().dfu3d_nms_normal_bev if normal else _lib.lib().dfu3d_nms_bev
        rc = fn(ctypes.c_void_p(boxes.data_ptr()), n, ctypes.c_float(0.2), ctypes.c_void_p(mask.data_ptr()),
                ctypes.c_void_p(keep.data_ptr()), ctypes.c_void_p(num.data_ptr()), st._stream())
        torch.cuda.synchronize()
        assert rc == -3                                                # DFU3D_ERANGE
        assert int(num.item()) == -7 and bool((keep == -1).all()) and not bool(mask.any())
