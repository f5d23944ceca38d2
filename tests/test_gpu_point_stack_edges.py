"""Edges of the stacked set-abstraction ops of csrc/pointstack_stage.hip: every kernel of the farthest-point-sampling
ladder on both sides of every boundary, tied maxima, the cap, every status bit, ball queries beyond one 64-slot fill and
one 256-row trip, clamped starts, short channel chunks, the second trip of the start scan, non-finite BEV coordinates, and
every entry point between guard bands with poisoned scratch.  Against the NumPy restatements of tests/point_stack_ref.py;
every comparison is an equality (of bits, for floats).

The kernel a farthest-point-sampling case launches is decided by the bound on a sample (cap if 1 <= cap < rows, else
rows), by the table of dfu3d_stk_fps, which is also dfu3d_pn2_fps's over N: shape_of() below restates it for the ids."""
import functools

import numpy as np
import pytest

from tests import point_stack_ref as R
from tests.test_gpu_point_stack import ball_ref, bits, cu, grid_case, with_status

pytestmark = pytest.mark.gpu

F32 = np.float32
K = R.FPS_K


def shape_of(bound):
    for top, name in ((256, "256x1"), (1024, "256x4"), (2048, "1024x2"), (4096, "1024x4"), (8192, "1024x8"),
                      (16384, "1024x16")):
        if bound <= top:
            return "k_stk_fps<%s>" % name.replace("x", ",")
    return "k_stk_fps_big"


def run_fps(xyz, start, npoint, cap=0):
    from dfu3d_amd import point_stack_ops as ops
    (idx, kp), st = with_status(ops.fps, cu(xyz), cu(np.asarray(start, np.int32)), npoint, cap=cap)
    return idx.cpu().numpy(), kp.cpu().numpy(), st


def inside(idx, per):
    """Every index of every sample lies inside the sample (index 0 for a sample without rows)."""
    return all(idx[b].min() >= 0 and idx[b].max() < max(n, 1) for b, n in enumerate(per))


# ---- farthest point sampling: every kernel, both sides of every boundary ----------------------------------------------------
FPS_TOTALS = [256, 257, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385]
FPS_TAIL = [1, 70, 0]


@pytest.mark.parametrize("total", FPS_TOTALS, ids=lambda t: "%d-%s" % (t, shape_of(t)))
def test_fps_every_kernel_shape_on_both_sides_of_every_boundary(total):
    """A lattice cloud (tied maxima at every step) of `total` rows as the only sample, then as sample 0 before samples of
    1, 70 and 0 rows, with cap = total so that the bound, and with it the kernel, stays that of `total`: the short samples
    cycle and the empty one zero-fills inside every kernel."""
    from dfu3d_amd import pointnet2_ops as pn2
    xyz, start = R.lattice_cloud(3000 + total, [total] + FPS_TAIL)
    ties = []
    R.fps_one(xyz[:total], K, ties)
    assert ties                                                              # otherwise the lattice proves nothing
    want_idx, want_kp, want_st = R.fps(xyz[:total], start[:2], K)
    idx, kp, st = run_fps(xyz[:total], start[:2], K)
    assert st == want_st == 0 and np.array_equal(idx, want_idx) and np.array_equal(bits(kp), bits(want_kp))
    alone, _ = pn2.fps(cu(xyz[None, :total]), K)                              # the batched op on that sample alone
    assert np.array_equal(alone.cpu().numpy()[0], idx[0])
    want_idx4, want_kp4, want_st4 = R.fps(xyz, start, K, cap=total)
    assert R.fps_bound(len(xyz), total) == total and np.array_equal(want_idx4[0], want_idx[0])
    idx4, kp4, st4 = run_fps(xyz, start, K, cap=total)
    assert st4 == want_st4 == R.ST_EMPTY
    assert np.array_equal(idx4, want_idx4) and np.array_equal(bits(kp4), bits(want_kp4))
    assert not idx4[1].any() and not idx4[3].any() and kp4[3 * K:].tolist() == [[3.0, 0.0, 0.0, 0.0]] * K
    assert np.array_equal(bits(kp4[K:2 * K, 1:]), bits(np.tile(xyz[total], (K, 1))))     # the one row, K times


# (cap, rows of the samples): the cap selects the kernel, sample 0 is beyond it
FPS_CAP_CASES = [(256, [300]), (1024, [1300, 5]), (2048, [2400]), (4096, [5000]), (8192, [9000, 40]), (16384, [17500]),
                 (17000, [20000, 100])]


@pytest.mark.parametrize("cap,per", FPS_CAP_CASES, ids=lambda v: shape_of(v) if isinstance(v, int) else str(sum(v)))
def test_fps_cap_cuts_a_longer_sample_in_every_kernel_shape(cap, per):
    """A sample beyond the cap: ST_BAD_COUNT, and the picks of its first `cap` rows -- those of the restatement with the
    cap, which are those of the restatement without one on the cloud with the other rows taken out.  A continuous cloud:
    sampled whole, it has picks at and beyond the cap, so a kernel that ignores the cap is seen in the picks too."""
    xyz, start = R.stacked_cloud(3100 + cap, per)
    whole = R.fps(xyz, start, K)
    assert whole[2] == 0 and whole[0][0].max() >= cap
    want_idx, want_kp, want_st = R.fps(xyz, start, K, cap=cap)
    cut = np.concatenate([xyz[:cap], xyz[per[0]:]])
    cut_idx, cut_kp, _ = R.fps(cut, R.starts([cap] + per[1:]), K)
    assert want_st == R.ST_BAD_COUNT and np.array_equal(want_idx, cut_idx) and np.array_equal(bits(want_kp), bits(cut_kp))
    idx, kp, st = run_fps(xyz, start, K, cap=cap)
    assert st == R.ST_BAD_COUNT
    assert idx[0].max() < cap
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(kp), bits(want_kp))


# (rows of the samples, K, the sample whose last row is non-finite)
FPS_BAD_POINT_CASES = [([300], 64, 0), ([5000], 64, 0), ([16500], 64, 0), ([16500], 1, 0), ([16500, 1], 8, 0),
                       ([16500, 1], 8, 1)]


@pytest.mark.parametrize("per,npoint,which", FPS_BAD_POINT_CASES, ids=str)
def test_fps_non_finite_coordinate_in_the_last_sampled_row_sets_bad_point(per, npoint, which):
    """The memory form (bound 16500 or 16501) finds the coordinate in the first step's walk; with one pick (K = 1, or the
    one-row sample of [16500, 1]) in the loop that exists only for this bit.  The picks are unspecified, but inside."""
    xyz, start = R.stacked_cloud(3200 + sum(per) + npoint, per)
    idx, kp, st = run_fps(xyz, start, npoint)
    want_idx, want_kp, want_st = R.fps(xyz, start, npoint)
    assert st == want_st == 0 and np.array_equal(idx, want_idx) and np.array_equal(bits(kp), bits(want_kp))
    row = int(start[which + 1]) - 1
    for col, bad in ((0, np.nan), (2, np.inf)):
        poisoned = xyz.copy()
        poisoned[row, col] = bad
        idx, kp, st = run_fps(poisoned, start, npoint)
        assert st == R.fps(poisoned, start, npoint)[2] == R.ST_BAD_POINT, (col, bad)
        assert inside(idx, per) and not idx[:, 0].any()
        other = 1 - which
        if len(per) > 1:                                                     # the clean sample keeps its picks
            assert np.array_equal(idx[other], want_idx[other])


@pytest.mark.parametrize("cap,per", [(256, [300]), (17000, [20000])], ids=["k_stk_fps<256,1>", "k_stk_fps_big"])
def test_fps_non_finite_coordinate_beyond_the_cap_is_not_looked_at(cap, per):
    """A row beyond the bound is not sampled, so a non-finite coordinate there raises nothing, in the register form and --
    since it is handed the bound -- in the memory form alike: its walks end at the bound.  The same value in the last row
    inside the bound is found."""
    xyz, start = R.stacked_cloud(3300 + cap, per)
    beyond = xyz.copy()
    beyond[cap + (per[0] - cap) // 2, 1] = np.nan
    want_idx, want_kp, want_st = R.fps(beyond, start, K, cap=cap)
    idx, kp, st = run_fps(beyond, start, K, cap=cap)
    assert st == want_st == R.ST_BAD_COUNT
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(kp), bits(want_kp))
    last = xyz.copy()
    last[cap - 1, 1] = np.inf
    idx, kp, st = run_fps(last, start, K, cap=cap)
    assert st == R.fps(last, start, K, cap=cap)[2] == R.ST_BAD_COUNT | R.ST_BAD_POINT and idx.max() < cap and idx.min() >= 0


def test_fps_ties_in_the_memory_form():
    """16500 and 90 rows on 125 lattice cells: every step of both samples has many equal maxima, in every wave."""
    per = R.FPS_BIG_COUNTS
    xyz, start = R.lattice_cloud(3400, per)
    for b in range(2):
        ties = []
        R.fps_one(xyz[start[b]:start[b + 1]], K, ties)
        assert len(ties) > K // 2
    want_idx, want_kp, want_st = R.fps(xyz, start, K)
    idx, kp, st = run_fps(xyz, start, K)
    assert st == want_st == 0 and np.array_equal(idx, want_idx) and np.array_equal(bits(kp), bits(want_kp))


# ---- counts and starts --------------------------------------------------------------------------------------------------------
def run_counts(column, B):
    from dfu3d_amd import point_stack_ops as ops
    (cnt, start), st = with_status(ops.counts, column, B)
    return cnt.cpu().numpy(), start.cpu().numpy(), st


def check_counts(col, B, status=None):
    want_cnt, want_start, want_st = R.counts(col, B)
    cnt, start, st = run_counts(cu(col), B)
    assert st == want_st and (status is None or st == status), (st, want_st, status)
    assert cnt.dtype == np.int32 and np.array_equal(cnt, want_cnt) and np.array_equal(start, want_start)
    return want_cnt


@pytest.mark.parametrize("B", [1025, 2049])
def test_counts_beyond_one_trip_of_the_start_scan(B):
    """k_stk_starts scans 1024 entries per trip: B = 1025 carries one entry into a second trip, B = 2049 into a third."""
    from dfu3d_amd import point_stack_ops as ops
    per = np.random.default_rng(B).choice([0, 1, 2, 65], B)
    per[[0, 1023, 1024, B - 1]] = [2, 65, 1, 2]
    col = np.repeat(np.arange(B), per)
    for dtype in (F32, np.int32):
        want = check_counts(col.astype(dtype), B, status=0)
        assert want.tolist() == per.tolist()
    start, st = with_status(ops.starts, cu(per.astype(np.int32)))
    assert st == 0 and np.array_equal(start.cpu().numpy(), R.starts(per))


@pytest.mark.parametrize("rows", [64, 128, 256, 512])
def test_counts_of_whole_waves_and_whole_workgroups(rows):
    for dtype in (F32, np.int32):
        for b in (0, 1):
            want = check_counts(np.full(rows, b, dtype), 2, status=0)
            assert want.tolist() == [rows * (1 - b), rows * b]


def test_counts_a_whole_wave_of_bad_rows():
    """Rows 64 .. 127 all hold B (or -1 in an int column): the wave's shared value is no sample, nothing is added for it,
    and the waves around it keep their counts."""
    B = 3
    col = np.r_[np.repeat([0, 1], [30, 34]), np.full(64, B)]
    for dtype in (F32, np.int32):
        want = check_counts(col.astype(dtype), B, status=R.ST_BAD_BATCH)
        assert want.tolist() == [30, 34, 0]
        behind = np.r_[col, np.repeat([1, 2], [10, 70])].astype(dtype)     # and rows behind the wave
        want = check_counts(behind, B, status=R.ST_BAD_BATCH | R.ST_UNSORTED)
        assert want.tolist() == [30, 44, 70]
    minus = np.r_[np.full(64, -1), np.repeat([0, 2], [64, 3])].astype(np.int32)
    assert check_counts(minus, B, status=R.ST_BAD_BATCH).tolist() == [64, 0, 3]


def test_counts_int_column_of_a_wider_block_with_bad_values():
    """indices[:, 0] of an int32 (N, 4) tensor, read in place with stride 4, one -1 and one B among the rows."""
    B = 4
    col = np.repeat(np.arange(B), [70, 3, 0, 130])
    col[5], col[100] = -1, B
    indices = np.random.default_rng(9).integers(-2, 50, (len(col), 4)).astype(np.int32)
    indices[:, 0] = col
    want_cnt, want_start, want_st = R.counts(col.astype(np.int32), B)
    assert want_cnt.tolist() == [69, 3, 0, 129] and want_st == R.ST_BAD_BATCH | R.ST_UNSORTED
    view = cu(indices)[:, 0]
    assert view.stride(0) == 4
    cnt, start, st = run_counts(view, B)
    assert st == want_st and np.array_equal(cnt, want_cnt) and np.array_equal(start, want_start)


def test_starts_takes_a_negative_count_as_zero():
    from dfu3d_amd import point_stack_ops as ops
    cnt = np.asarray([5, -3, 7], np.int32)
    start, st = with_status(ops.starts, cu(cnt))
    assert start.cpu().tolist() == [0, 5, 5, 12] == R.starts(cnt).tolist() and st == R.starts_status(cnt) == R.ST_BAD_COUNT


# ---- ball query ---------------------------------------------------------------------------------------------------------------
def run_ball(xyz, start, ctr, cstart, radii, nsamples):
    from dfu3d_amd import point_stack_ops as ops
    res, st = with_status(ops.ball_query, cu(xyz), cu(np.asarray(start, np.int32)), cu(ctr),
                          cu(np.asarray(cstart, np.int32)), radii, nsamples)
    return [(i.cpu().numpy(), e.cpu().numpy()) for i, e in res], st


def check_ball(xyz, start, ctr, cstart, radius, nsample, status=0):
    want_idx, want_empty, want_st = R.ball_query(xyz, start, ctr, cstart, radius, nsample, with_status=True)
    ((idx, empty),), st = run_ball(xyz, start, ctr, cstart, [radius], [nsample])
    assert st == want_st == status
    assert idx.shape == (len(ctr), nsample) and np.array_equal(idx, want_idx) and np.array_equal(empty, want_empty)
    return idx, empty


@functools.lru_cache(maxsize=None)
def dense_case():
    """700 and 30 lattice points (125 cells); centre 0 at the origin has more than 130 hits inside 0.5, centre 1 on a face
    of the lattice between 65 and 129, centre 2 at a corner fewer than 64, centre 3 none; two centres over sample 1."""
    xyz, start = R.lattice_cloud(3500, [700, 30])
    ctr = np.asarray([[0, 0, 0], [0.5, 0, 0], [0.5, 0.5, 0.5], [30, 0, 0], [0, 0, 0], [0.5, 0.5, -0.5]], F32)
    cstart = np.asarray([0, 4, 6], np.int32)
    hits = (R.sqdist(ctr[:4, None, :], xyz[None, :700, :]) < F32(0.25)).sum(1)
    assert hits[0] > 130 and 65 <= hits[1] <= 129 and 0 < hits[2] < 64 and hits[3] == 0, hits
    return xyz, start, ctr, cstart


@pytest.mark.parametrize("nsample", [64, 65, 130])
def test_ball_query_fills_beyond_one_pass_of_64_slots(nsample):
    """nsample above 64: a scale needs a second 64-row tile (and a second 256-row trip) to fill, and the loop that writes
    the first hit into the remaining slots takes more than one pass.  Alone, and as scale 1 beside a scale 0 of four slots
    that is full after the first tile while scale 1 walks on."""
    xyz, start, ctr, cstart = dense_case()
    idx, empty = check_ball(xyz, start, ctr, cstart, 0.5, nsample)
    assert empty[:4].tolist() == [0, 0, 0, 1] and idx[0, -1] > idx[0, 0] and (idx[2, 64:] == idx[2, 0]).all()
    small = R.ball_query(xyz, start, ctr, cstart, 0.5, 4)
    both, st = run_ball(xyz, start, ctr, cstart, [0.5, 0.5], [4, nsample])
    assert st == 0 and np.array_equal(both[0][0], small[0]) and np.array_equal(both[0][1], small[1])
    assert np.array_equal(both[1][0], idx) and np.array_equal(both[1][1], empty)


def test_ball_query_only_hit_in_the_last_row_of_a_sample():
    """Samples of 255, 256, 257, 512 and 513 rows, all far away but the last: every 256-row trip is walked, the first hit
    is the last row, and every slot carries it."""
    per = [255, 256, 257, 512, 513]
    xyz = np.random.default_rng(36).uniform(40.0, 60.0, (sum(per), 3)).astype(F32)
    start = R.starts(per)
    xyz[start[1:] - 1] = [0.25, 0.0, 0.0]
    ctr, cstart = np.zeros((len(per), 3), F32), np.arange(len(per) + 1, dtype=np.int32)
    idx, empty = check_ball(xyz, start, ctr, cstart, 0.5, 3)
    assert not empty.any() and idx.tolist() == [[n - 1] * 3 for n in per]


def test_ball_query_radius_zero_negative_and_infinite():
    per = [1, 63, 65]
    xyz, start = R.lattice_cloud(3600, per)
    ctr = np.concatenate([xyz[[0, 1, 64]], [[0.125, 0, 0]] * 3]).astype(F32)      # three coincide with a point
    cstart = np.asarray([0, 2, 4, 6], np.int32)
    ctr = ctr[[0, 3, 1, 4, 2, 5]]
    idx, empty = check_ball(xyz, start, ctr, cstart, 0.0, 5)                        # strict: not even distance 0 is a hit
    assert empty.all() and not idx.any()
    plus, _ = check_ball(xyz, start, ctr, cstart, 0.5, 70)
    minus, _ = check_ball(xyz, start, ctr, cstart, -0.5, 70)                        # the radius enters as its square
    assert np.array_equal(plus, minus)
    idx, empty = check_ball(xyz, start, ctr, cstart, float('inf'), 70)             # every row of the sample, no padded lane
    for m, n in enumerate(np.repeat(per, 2)):
        assert idx[m].tolist() == list(range(n)) + [0] * (70 - n) and not empty[m]


def test_ball_query_centres_beyond_the_last_sample_and_clamped_starts():
    xyz, start, ctr, cstart = grid_case()
    short = cstart.copy()
    short[-1] -= 2                                                                  # two centres belong to no sample
    idx, empty = check_ball(xyz, start, ctr, short, 0.5, 16, status=R.ST_BAD_COUNT)
    assert empty[-2:].all() and not idx[-2:].any()
    assert np.array_equal(idx[:-2], ball_ref(0.5, 16)[0][:-2])
    bad = start.copy()                              # [0, 0, 1, 64, 128, 193, 893]
    bad[2], bad[-1] = 70, len(xyz) + 50             # sample 1 longer, sample 2 descending (no rows), the end beyond N
    assert bad[3] < bad[2] and R.sample_rows(bad, 2, len(xyz))[1] == 0
    idx, empty = check_ball(xyz, bad, ctr, cstart, 0.5, 16, status=R.ST_BAD_COUNT)
    assert empty[int(cstart[2]):int(cstart[3])].all()
    assert np.array_equal(idx[int(cstart[5]):], ball_ref(0.5, 16)[0][int(cstart[5]):])   # clamped to the rows there are


def test_ball_query_without_points_and_without_centres():
    ctr = np.zeros((5, 3), F32)
    idx, empty = check_ball(np.zeros((0, 3), F32), [0, 0, 0], ctr, [0, 2, 5], 0.5, 4)
    assert empty.all() and not idx.any()
    xyz, start = R.lattice_cloud(3700, [40, 9])
    res, st = run_ball(xyz, start, np.zeros((0, 3), F32), [0, 0, 0], [0.5, 1.0], [4, 70])
    assert st == 0 and [(i.shape, e.shape) for i, e in res] == [((0, 4), (0,)), ((0, 70), (0,))]


# ---- grouping and its backward --------------------------------------------------------------------------------------------------
def payload_features(seed, N, C):
    raw = np.random.default_rng(seed).integers(0, 2 ** 32, (N, C), dtype=np.uint64).astype(np.uint32)
    raw[::3] |= 0x7FC00000                                                          # NaNs with payloads among them
    return raw.view(F32)


def run_group(xyz, start, ctr, cstart, feat, idx, empty):
    from dfu3d_amd import point_stack_ops as ops
    t = lambda a: None if a is None else cu(a)                                      # noqa: E731
    out, st = with_status(ops.group, t(xyz), cu(np.asarray(start, np.int32)), t(ctr), cu(np.asarray(cstart, np.int32)),
                          t(feat), cu(idx), cu(empty))
    return out.cpu().numpy(), st


@pytest.mark.parametrize("C,plain", [(15, False), (17, False), (33, False), (17, True)])
def test_group_short_last_chunk_of_channels(C, plain):
    """Channels go to workgroups in chunks of 16: a last chunk of 15 channels, of 1, and of 1 behind two full ones."""
    xyz, start, ctr, cstart = grid_case()
    idx, empty = ball_ref(0.5, 16)
    feat = payload_features(C, len(xyz), C)
    pts, centres = (None, None) if plain else (xyz, ctr)
    want, want_st = R.group(pts, start, centres, cstart, feat, idx, empty, with_status=True)
    out, st = run_group(pts, start, centres, cstart, feat, idx, empty)
    assert st == want_st == 0 and out.shape == ((0 if plain else 3) + C, len(ctr), 16)
    assert np.array_equal(bits(out), bits(want)) and not bits(out)[:, empty == 1].any()


@pytest.mark.parametrize("M,ns", [(85, 3), (64, 4), (257, 1)], ids=["255", "256", "257"])
def test_group_entries_around_one_workgroup(M, ns):
    xyz, start = R.lattice_cloud(3800 + M, [100, 60])
    ctr, cstart = R.lattice_cloud(3900 + M, [M - 20, 20])
    ctr[::9] += F32(30.0)
    idx, empty = R.ball_query(xyz, start, ctr, cstart, 0.5, ns)
    assert empty.any() and not empty.all()
    feat = payload_features(M, len(xyz), 2)
    want, want_st = R.group(xyz, start, ctr, cstart, feat, idx, empty, with_status=True)
    out, st = run_group(xyz, start, ctr, cstart, feat, idx, empty)
    assert st == want_st == 0 and np.array_equal(bits(out), bits(want))


def test_group_and_backward_with_centres_beyond_the_last_sample_and_clamped_starts():
    """Two centres at and beyond cstart[B]: zeros forward, -1 in the global index (so left out of the backward) and
    ST_BAD_COUNT from each of the three calls; then starts that need clamping, against the restatement on the clamped
    ones."""
    from dfu3d_amd import point_stack_ops as ops
    xyz, start, ctr, cstart = grid_case()
    N, C = len(xyz), 5
    short = cstart.copy()
    short[-1] -= 2
    idx, empty, st = R.ball_query(xyz, start, ctr, short, 0.5, 16, with_status=True)
    assert st == R.ST_BAD_COUNT and empty[-2:].all()
    rng = np.random.default_rng(39)
    feat = rng.normal(size=(N, C)).astype(F32)
    want, want_st = R.group(xyz, start, ctr, short, feat, idx, empty, with_status=True)
    out, st = run_group(xyz, start, ctr, short, feat, idx, empty)
    assert st == want_st == R.ST_BAD_COUNT and np.array_equal(bits(out), bits(want)) and not bits(out)[:, -2:].any()
    want_gidx, want_st = R.global_index(start, short, idx, empty, N)
    gidx, st = with_status(ops.global_index, cu(idx), cu(empty), cu(start), cu(short), N)
    assert st == want_st == R.ST_BAD_COUNT and np.array_equal(gidx.cpu().numpy().reshape(-1), want_gidx)
    assert (want_gidx.reshape(len(ctr), 16)[-2:] == -1).all()
    grad = rng.normal(size=(3 + C, len(ctr), 16)).astype(F32)
    want_gf, want_st = R.group_backward(grad, start, short, idx, empty, N, with_status=True)
    gf, st = with_status(ops.group_backward, cu(grad), cu(idx), cu(empty), cu(start), cu(short), N)
    assert st == want_st == R.ST_BAD_COUNT and np.array_equal(bits(gf.cpu().numpy()), bits(want_gf))
    # the same two centres marked as balls with hits: their indices are outside a sample without rows
    hit = empty.copy()
    hit[-2:] = 0
    want, want_st = R.group(xyz, start, ctr, short, feat, idx, hit, with_status=True)
    out, st = run_group(xyz, start, ctr, short, feat, idx, hit)
    assert st == want_st == R.ST_BAD_COUNT | R.ST_BAD_INDEX and np.array_equal(bits(out), bits(want))
    gidx, st = with_status(ops.global_index, cu(idx), cu(hit), cu(start), cu(short), N)
    assert st == R.ST_BAD_COUNT | R.ST_BAD_INDEX and np.array_equal(gidx.cpu().numpy().reshape(-1), want_gidx)
    # clamped starts
    bad = start.copy()
    bad[2], bad[-1] = 70, N + 50
    idx, empty, st = R.ball_query(xyz, bad, ctr, cstart, 0.5, 16, with_status=True)
    want, want_st = R.group(xyz, bad, ctr, cstart, feat, idx, empty, with_status=True)
    out, st = run_group(xyz, bad, ctr, cstart, feat, idx, empty)
    assert st == want_st == R.ST_BAD_COUNT and np.array_equal(bits(out), bits(want))
    want_gf, want_st = R.group_backward(grad, bad, cstart, idx, empty, N, with_status=True)
    gf, st = with_status(ops.group_backward, cu(grad), cu(idx), cu(empty), cu(bad), cu(cstart), N)
    assert st == want_st == R.ST_BAD_COUNT and np.array_equal(bits(gf.cpu().numpy()), bits(want_gf))


# ---- bilinear BEV sampling ------------------------------------------------------------------------------------------------------
BEV_RANGE, BEV_VOXEL, BEV_STRIDE = [-1.4, -1.0, -1.0], [0.1, 0.1, 0.2], 2           # one cell of the map is 0.2 m


def check_bev(kp, spatial, voxel=BEV_VOXEL, status=0, stride=BEV_STRIDE):
    """Bits against the restatement; where the restatement is NaN (an infinite weight: inf - inf, 0 * inf) any NaN, since
    IEEE 754 leaves the sign and payload of that NaN open."""
    from dfu3d_amd import point_stack_ops as ops
    want, want_st = R.bev_sample(kp, spatial, BEV_RANGE, voxel, stride, with_status=True)
    out, st = with_status(ops.bev_sample, cu(kp), cu(spatial), BEV_RANGE, voxel, stride)
    out = out.cpu().numpy()
    assert st == want_st == status and out.shape == want.shape
    assert R.same_bits_or_nan(out, want)
    return out


def bev_keypoints(rng, M, B):
    xy = rng.uniform([-1.8, -1.4], [0.4, 0.4], (M, 2))                              # inside the map and around it
    return np.concatenate([rng.integers(0, B, (M, 1)), xy, rng.normal(size=(M, 1))], 1).astype(F32)


def test_bev_sample_non_finite_coordinates():
    """NaN, +inf and -inf in x and in y: index 0 on that axis for both neighbours (the reference's floor().long() of a
    non-finite value is the most negative integer on the host, and so is that + 1; clamp makes both 0).  The row is NaN
    in every channel, as the reference's is: the weights of the axis are infinite and of opposite sign."""
    rng = np.random.default_rng(40)
    B, C, H, W = 2, 3, 5, 7
    spatial = rng.normal(size=(B, C, H, W)).astype(F32)
    kp = bev_keypoints(rng, 12, B)
    for i, (col, bad) in enumerate((c, v) for c in (1, 2) for v in (np.nan, np.inf, -np.inf)):
        kp[2 * i, col] = bad
    out = check_bev(kp, spatial)
    assert np.isnan(out[:12:2]).all() and np.isfinite(out[1:12:2]).all()
    tiny = [1e-30, 0.1, 0.2]                               # with a stride as small, fx overflows for ordinary x (no denormal)
    kp = bev_keypoints(rng, 9, B)
    with np.errstate(all='ignore'):
        assert np.isinf(((kp[:, 1] - F32(BEV_RANGE[0])) / F32(tiny[0])) / F32(1e-30)).all()
    assert np.isnan(check_bev(kp, spatial, voxel=tiny, stride=1e-30)).all()


@pytest.mark.parametrize("H,W", [(1, 7), (5, 1), (1, 1)])
def test_bev_sample_maps_of_one_row_or_one_column(H, W):
    rng = np.random.default_rng(41 + H + W)
    B, C = 2, 4
    spatial = rng.normal(size=(B, C, H, W)).astype(F32)
    kp = bev_keypoints(rng, 50, B)
    kp[:4, 1:3] = [[-1.4, -1.0], [-1.3, -0.9], [-1.4 + 0.2 * (W - 1), -1.0 + 0.2 * (H - 1)], [-1.5, -1.1]]
    out = check_bev(kp, spatial)
    # one row: y0 = y1, the two weights of a column are p and -p on the same value and cancel exactly (a signed zero);
    # one column: the cancelling terms are not neighbours in the sum, and what rounding leaves is compared bit for bit
    assert out.any() == (W == 1 and H > 1)


def test_bev_sample_fractional_and_negative_zero_sample_index():
    rng = np.random.default_rng(43)
    B, C, H, W = 2, 3, 5, 7
    spatial = rng.normal(size=(B, C, H, W)).astype(F32)
    kp = bev_keypoints(rng, 10, B)
    kp[:, 1:3] = np.clip(kp[:, 1:3], [-1.3, -0.9], [-0.3, -0.3])                    # inside the map: the weights are not zero
    kp[0, 0], kp[1, 0], kp[2, 0] = 0.5, -0.0, B
    out = check_bev(kp, spatial, status=R.ST_BAD_BATCH)
    assert not out[0].any() and not out[2].any() and out[1].any()
    zero = kp.copy()
    zero[1, 0] = 0.0
    assert np.array_equal(bits(out[1]), bits(R.bev_sample(zero, spatial, BEV_RANGE, BEV_VOXEL, BEV_STRIDE)[1]))   # sample 0
    check_bev(kp[[1, 3, 4, 5, 6]], spatial)                                          # -0.0 alone raises nothing


@pytest.mark.parametrize("M", [256, 257, 1])
def test_bev_sample_one_channel_around_one_workgroup(M):
    rng = np.random.default_rng(44 + M)
    spatial = rng.normal(size=(2, 1, 5, 7)).astype(F32)
    out = check_bev(bev_keypoints(rng, M, 2), spatial)
    assert out.shape == (M, 1) and out.any()


# ---- guard bands and poisoned scratch ---------------------------------------------------------------------------------------------
def status_word():
    import torch
    return torch.zeros(1, dtype=torch.int32, device='cuda')


def test_guard_bands_counts():
    from dfu3d_amd import point_stack_ops as ops
    from tests.test_gpu_guard_bands import both_poisons
    B = 5
    col = np.repeat(np.arange(B), [130, 0, 67, 1, 256])
    points = np.random.default_rng(50).normal(size=(len(col), 5)).astype(F32)
    points[:, 0] = col
    indices = np.random.default_rng(51).integers(0, 40, (len(col), 4)).astype(np.int32)
    indices[:, 0] = col
    want = R.counts(col, B)

    def run():
        st = status_word()
        with ops.status_scope(st):
            a, b = ops.counts(cu(points)[:, 0], B), ops.counts(cu(indices)[:, 0], B)
            c = ops.starts(cu(want[0]))
        return list(a) + list(b) + [c, st]

    def verify(out):
        for k in (0, 2):
            assert np.array_equal(out[k], want[0]) and np.array_equal(out[k + 1], want[1])
        assert np.array_equal(out[4], want[1]) and out[5].tolist() == [0]
    both_poisons(run, verify)


@pytest.mark.parametrize("per", [[300], [5000], R.FPS_BIG_COUNTS], ids=str)
def test_guard_bands_fps(per):
    """The scratch of the memory form arrives poisoned (NaN, then zeros): the first step must not read it."""
    from dfu3d_amd import point_stack_ops as ops
    from tests.test_gpu_guard_bands import both_poisons
    xyz, start = R.stacked_cloud(5200 + sum(per), per)
    want_idx, want_kp, want_st = R.fps(xyz, start, K)
    assert want_st == 0

    def run():
        st = status_word()
        with ops.status_scope(st):
            idx, kp = ops.fps(cu(xyz), cu(start), K)
        return idx, kp, st

    def verify(out):
        assert np.array_equal(out[0], want_idx) and np.array_equal(bits(out[1]), bits(want_kp)) and out[2].tolist() == [0]
    both_poisons(run, verify, min_count=4 + (sum(per) > 16384))


def test_guard_bands_ball_query():
    from dfu3d_amd import point_stack_ops as ops
    from tests.test_gpu_guard_bands import both_poisons
    xyz, start, ctr, cstart = grid_case()
    want = [ball_ref(0.5, 16), ball_ref(1.0, 32), ball_ref(0.5, 1)]

    def run():
        st = status_word()
        args = (cu(xyz), cu(start), cu(ctr), cu(cstart))
        with ops.status_scope(st):
            two = ops.ball_query(*args, [0.5, 1.0], [16, 32])
            one = ops.ball_query(*args, [0.5], [1])
        return [list(p) for p in two + one] + [st]

    def verify(out):
        for got, w in zip(out, want):
            assert np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1])
        assert out[3].tolist() == [0]
    both_poisons(run, verify, min_count=8)


def test_guard_bands_group():
    from dfu3d_amd import point_stack_ops as ops
    from tests.test_gpu_guard_bands import both_poisons
    xyz, start, ctr, cstart = grid_case()
    idx, empty = ball_ref(0.5, 16)
    feat = payload_features(52, len(xyz), 17)
    want = [R.group(xyz, start, ctr, cstart, None, idx, empty), R.group(xyz, start, ctr, cstart, feat, idx, empty),
            R.group(None, start, None, cstart, feat, idx, empty)]

    def run():
        st = status_word()
        t_start, t_cstart, t_idx, t_empty, t_feat = cu(start), cu(cstart), cu(idx), cu(empty), cu(feat)
        with ops.status_scope(st):
            return [ops.group(cu(xyz), t_start, cu(ctr), t_cstart, None, t_idx, t_empty),
                    ops.group(cu(xyz), t_start, cu(ctr), t_cstart, t_feat, t_idx, t_empty),
                    ops.group(None, t_start, None, t_cstart, t_feat, t_idx, t_empty), st]

    def verify(out):
        for got, w in zip(out, want):
            assert np.array_equal(bits(got), bits(w))
        assert out[3].tolist() == [0]
    both_poisons(run, verify, min_count=9)


def test_guard_bands_query_group_backward():
    from dfu3d_amd import point_stack_ops as ops
    from tests.test_gpu_guard_bands import both_poisons
    xyz, start, ctr, cstart = grid_case()
    idx, empty = ball_ref(1.0, 32)
    N, C = len(xyz), 5
    rng = np.random.default_rng(53)
    feat = rng.normal(size=(N, C)).astype(F32)
    grad = rng.normal(size=(3 + C, len(ctr), 32)).astype(F32)
    want_out = R.group(xyz, start, ctr, cstart, feat, idx, empty)
    want_grad = R.group_backward(grad, start, cstart, idx, empty, N)

    def run():
        st = status_word()
        f = cu(feat).requires_grad_(True)
        with ops.status_scope(st):
            out = ops.query_group(cu(xyz), cu(start), cu(ctr), cu(cstart), f, cu(idx), cu(empty))
            out.backward(cu(grad))
        return out, f.grad, st

    def verify(out):
        assert np.array_equal(bits(out[0]), bits(want_out)) and np.array_equal(bits(out[1]), bits(want_grad))
        assert out[2].tolist() == [0]
    both_poisons(run, verify, min_count=8)


def test_guard_bands_bev_sample():
    from dfu3d_amd import point_stack_ops as ops
    from tests.test_gpu_guard_bands import both_poisons
    rng = np.random.default_rng(54)
    spatial = rng.normal(size=(2, 70, 5, 7)).astype(F32)
    kp = bev_keypoints(rng, 61, 2)
    kp[:3, 1:3] = [[-1.4, -1.0], [-0.2, -0.2], [5.0, -5.0]]
    want = R.bev_sample(kp, spatial, BEV_RANGE, BEV_VOXEL, BEV_STRIDE)
    assert np.isfinite(want).all()

    def run():
        st = status_word()
        with ops.status_scope(st):
            return ops.bev_sample(cu(kp), cu(spatial), BEV_RANGE, BEV_VOXEL, BEV_STRIDE), st

    def verify(out):
        assert np.array_equal(bits(out[0]), bits(want)) and out[1].tolist() == [0]
    both_poisons(run, verify, min_count=3)
