"""The restatements of tests/point_stack_ref.py against something plainer, without a GPU: farthest point sampling in
float64 on a lattice cloud (exact inputs, so the float32 restatement must give the same picks, and the maxima tie), and
the cap, clamped-start, beyond-cstart[B] and non-finite rules of csrc/dfu3d_stk.h on hand-written cases."""
import numpy as np
import pytest

from tests import point_stack_ref as R

F32 = np.float32


@pytest.mark.parametrize("n", [257, 2049, 4097])
def test_float64_fps_on_the_lattice_equals_the_restatement_and_the_maxima_tie(n):
    xyz, start = R.lattice_cloud(400 + n, [n])
    assert start.tolist() == [0, n] and xyz.dtype == F32 and len(np.unique(xyz, axis=0)) < n      # duplicates
    assert np.array_equal(xyz * 4, np.round(xyz * 4)) and np.abs(xyz).max() <= 0.5
    d2 = R.sqdist(xyz[:, None, :], xyz[None, :64, :])
    assert np.array_equal(d2.astype(np.float64), ((xyz[:, None].astype(np.float64) - xyz[None, :64]) ** 2).sum(-1))  # exact
    ties = []
    want = R.fps_one(xyz, 64, ties)
    assert np.array_equal(R.fps_plain64(xyz, 64), want)
    assert len(ties) >= 1 and want.max() > 0
    idx, kp, st = R.fps(xyz, start, 64)
    assert st == 0 and np.array_equal(idx[0], want) and np.array_equal(kp[:, 1:], xyz[want])


def test_counts_vectorised_rules():
    cnt, start, st = R.counts(np.asarray([0, 0, 2, 2, 2, 3], F32), 4)
    assert cnt.tolist() == [2, 0, 3, 1] and start.tolist() == [0, 2, 2, 5, 6] and st == 0 and cnt.dtype == np.int32
    for col, want, bits in (([0, 1, 0], [2, 1], R.ST_UNSORTED), ([0, 2, 1], [1, 1], R.ST_BAD_BATCH | R.ST_UNSORTED),
                            ([-1, 0, 0.5, 1], [1, 1], R.ST_BAD_BATCH), ([0, np.nan, 1], [1, 1], R.ST_BAD_BATCH),
                            ([0, 1, np.inf], [1, 1], R.ST_BAD_BATCH)):
        cnt, _, st = R.counts(np.asarray(col, F32), 2)
        assert cnt.tolist() == want and st == bits, col
    cnt, start, st = R.counts(np.asarray([-1, 0, 2, 1], np.int32), 2)
    assert cnt.tolist() == [1, 1] and st == R.ST_BAD_BATCH | R.ST_UNSORTED
    assert R.starts([5, -3, 7]).tolist() == [0, 5, 5, 12] and R.starts_status([5, -3, 7]) == R.ST_BAD_COUNT
    assert R.starts_status([5, 0, 7]) == 0


def test_sample_rows_clamps_as_the_header_states():
    S = R.sample_rows
    assert S([0, 5, 9], 0, 9) == (0, 5, 0) and S([0, 5, 9], 1, 9) == (5, 4, 0)
    assert S([0, 5, 12], 1, 9) == (5, 4, R.ST_BAD_COUNT)                     # the end beyond the rows
    assert S([0, 7, 4], 1, 9) == (7, 0, R.ST_BAD_COUNT)                      # descending: no rows
    assert S([-3, 4], 0, 9) == (0, 4, R.ST_BAD_COUNT) and S([11, 12], 0, 9) == (9, 0, R.ST_BAD_COUNT)


def test_fps_cap_clamp_and_non_finite_rules():
    xyz = np.asarray([[0, 0, 0], [1, 0, 0], [5, 0, 0], [2, 0, 0], [9, 0, 0], [3, 0, 0]], F32)
    idx, kp, st = R.fps(xyz, [0, 6], 3)
    assert idx.tolist() == [[0, 4, 2]] and st == 0
    assert R.fps_bound(6, 0) == 6 and R.fps_bound(6, 6) == 6 and R.fps_bound(6, 5) == 5 and R.fps_bound(6, 9) == 6
    idx, kp, st = R.fps(xyz, [0, 6], 3, cap=4)                              # rows 4 and 5 are not sampled
    assert idx.tolist() == [[0, 2, 3]] and st == R.ST_BAD_COUNT and np.array_equal(kp[:, 1:], xyz[[0, 2, 3]])
    assert R.fps(xyz, [0, 6], 3, cap=6)[2] == 0 and R.fps(xyz, [0, 4, 6], 3, cap=4)[2] == 0
    idx, kp, st = R.fps(xyz, [0, 4, 9], 3)                                  # the end beyond the rows: clamped to 6
    assert idx.tolist() == [[0, 2, 3], [0, 1, 0]] and st == R.ST_BAD_COUNT  # the two-row sample cycles
    idx, kp, st = R.fps(xyz, [0, 4, 9], 3, rows=5)                          # and to the rows the call is told of
    assert idx.tolist() == [[0, 2, 3], [0, 0, 0]] and st == R.ST_BAD_COUNT
    idx, kp, st = R.fps(xyz, [0, 6, 6], 2)
    assert st == R.ST_EMPTY and idx[1].tolist() == [0, 0] and kp[2:].tolist() == [[1, 0, 0, 0]] * 2
    for bad in (np.nan, np.inf, -np.inf):
        poisoned = xyz.copy()
        poisoned[5, 1] = bad
        idx, _, st = R.fps(poisoned, [0, 6], 3)
        assert st == R.ST_BAD_POINT and 0 <= idx.min() and idx.max() < 6
        idx, _, st = R.fps(poisoned, [0, 6], 3, cap=5)                      # the row is beyond the bound: not looked at
        assert st == R.ST_BAD_COUNT and idx.tolist() == [[0, 4, 2]]


def test_ball_query_group_and_backward_rules():
    xyz = np.asarray([[0, 0, 0], [0.25, 0, 0], [9, 9, 9], [0, 0, 0.25], [0, 0, 0]], F32)
    ctr = np.asarray([[0, 0, 0], [0, 0, 0], [0, 0, 0]], F32)
    start, cstart = np.asarray([0, 3, 5], np.int32), np.asarray([0, 1, 2], np.int32)
    idx, empty, st = R.ball_query(xyz, start, ctr, cstart, 0.5, 3, with_status=True)
    assert idx.tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 0]] and empty.tolist() == [0, 0, 1] and st == R.ST_BAD_COUNT
    assert R.ball_query(xyz, start, ctr[:2], cstart, 0.5, 3, with_status=True)[2] == 0
    assert R.ball_query(xyz, start, ctr[:2], cstart, 0.0, 3)[1].tolist() == [1, 1]        # strict: no hit at distance 0
    assert np.array_equal(R.ball_query(xyz, start, ctr[:2], cstart, -0.5, 3)[0], idx[:2])
    assert R.ball_query(xyz, start, ctr[:2], cstart, np.inf, 4)[0].tolist() == [[0, 1, 2, 0], [0, 1, 0, 0]]
    bad = np.asarray([0, 4, 7], np.int32)                                                # sample 1: rows 4 .. 5 after the clamp
    idx2, empty2, st2 = R.ball_query(xyz, bad, ctr[:2], cstart, 0.5, 3, with_status=True)
    assert idx2.tolist() == [[0, 1, 3], [0, 0, 0]] and empty2.tolist() == [0, 0] and st2 == R.ST_BAD_COUNT
    feat = np.arange(10, dtype=F32).reshape(5, 2)
    out, st = R.group(xyz, start, ctr, cstart, feat, idx, empty, with_status=True)
    assert st == R.ST_BAD_COUNT and out.shape == (5, 3, 3) and not out[:, 2].any()
    assert out[3:, 1].tolist() == [[6, 8, 6], [7, 9, 7]] and out[0, 0].tolist() == [0, 0.25, 0]
    plain, st = R.group(None, start, None, cstart, feat, idx[:2], empty[:2], with_status=True)
    assert st == 0 and np.array_equal(plain, out[3:, :2])
    far = idx.copy()
    far[1, 2] = 2                                                                        # sample 1 has two rows
    out2, st = R.group(xyz, start, ctr[:2], cstart, feat, far[:2], empty[:2], with_status=True)
    assert st == R.ST_BAD_INDEX and np.array_equal(out2, out[:, :2])                     # row 0 of the sample was read
    gidx, st = R.global_index(start, cstart, idx, empty, 5)
    assert gidx.tolist() == [0, 1, 0, 3, 4, 3, -1, -1, -1] and st == R.ST_BAD_COUNT
    gidx, st = R.global_index(start, cstart, far[:2], empty[:2], 5)
    assert gidx.tolist() == [0, 1, 0, 3, 4, -1] and st == R.ST_BAD_INDEX
    grad = np.ones((5, 3, 3), F32)
    gf, st = R.group_backward(grad, start, cstart, idx, empty, 5, with_status=True)
    assert st == R.ST_BAD_COUNT and gf.tolist() == [[2, 2], [1, 1], [0, 0], [2, 2], [1, 1]]


def test_bev_sample_status_and_non_finite_rule():
    sp = np.arange(2 * 1 * 2 * 3, dtype=F32).reshape(2, 1, 2, 3) + 1
    args = ([0.0, 0.0, 0.0], [1.0, 1.0, 1.0], 1)
    kp = np.asarray([[0, 1.5, 0.5, 0], [1, 0, 0, 0], [2, 0, 0, 0], [0.5, 0, 0, 0], [-0.0, 1, 0, 0], [np.nan, 0, 0, 0]], F32)
    out, st = R.bev_sample(kp, sp, *args, with_status=True)
    assert st == R.ST_BAD_BATCH and out[:, 0].tolist() == [4.0, 7.0, 0.0, 0.0, 2.0, 0.0]
    assert R.bev_sample(kp[:2], sp, *args, with_status=True)[1] == 0
    assert [R.clamp_floor(F32(v), 6) for v in (np.nan, np.inf, -np.inf, -2.0, 3.0, 6.0, 7.0, 1e30)] == [0, 0, 0, 0, 3, 6, 6, 6]
    for bad in (np.nan, np.inf, -np.inf):
        for col in (1, 2):
            k = np.asarray([[0, 1.0, 1.0, 0]], F32)
            k[0, col] = bad
            assert np.isnan(R.bev_sample(k, sp, *args)).all()        # the weights of the axis are infinite: inf - inf
    assert R.same_bits_or_nan(np.asarray([np.nan, 1.0], F32), -np.asarray([np.nan, -1.0], F32))
    assert not R.same_bits_or_nan(np.asarray([0.0], F32), np.asarray([-0.0], F32))
    assert not R.same_bits_or_nan(np.asarray([np.nan], F32), np.asarray([1.0], F32))
