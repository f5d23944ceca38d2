"""The stacked set-abstraction ops of csrc/pointstack_stage.hip on the GPU, against the NumPy float32 restatements of
tests/point_stack_ref.py and the batched ops of pointnet2_ops.  Every comparison is an equality."""
import functools

import numpy as np
import pytest

from tests import point_stack_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def with_status(fn, *args, **kwargs):
    """fn(*args) inside a status scope -> (result, status bits)."""
    import torch
    from dfu3d_amd import point_stack_ops as ops
    st = torch.zeros(1, dtype=torch.int32, device='cuda')
    with ops.status_scope(st):
        res = fn(*args, **kwargs)
    return res, int(st.item())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- counts -------------------------------------------------------------------------------------------------------------
def test_counts_float_and_int_columns_with_an_empty_sample():
    from dfu3d_amd import point_stack_ops as ops
    per = [130, 0, 67, 1]                                                   # more than one wave, an empty middle sample
    col = np.repeat(np.arange(4), per)
    points = np.random.default_rng(5).normal(size=(len(col), 5)).astype(F32)
    points[:, 0] = col
    indices = np.random.default_rng(6).integers(0, 40, (len(col), 4)).astype(np.int32)
    indices[:, 0] = col
    for column in (cu(points)[:, 0], cu(indices)[:, 0], cu(col.astype(F32)), cu(col.astype(np.int32))):
        (cnt, start), st = with_status(ops.counts, column, 4)
        assert st == 0 and cnt.dtype == start.dtype and cnt.cpu().tolist() == per
        assert start.cpu().tolist() == [0, 130, 130, 197, 198]
        assert ops.starts_of(cnt) is start                                  # kept on the count tensor
        assert np.array_equal(ops.starts(cnt).cpu().numpy(), R.starts(per))
    want = R.counts(col, 4)
    assert want[0].tolist() == per and want[2] == 0


def test_counts_status_bits():
    from dfu3d_amd import point_stack_ops as ops
    col = np.repeat(np.arange(3), [70, 5, 60]).astype(F32)
    for bad, bit in ((np.r_[col[:80], 0, col[80:]], R.ST_UNSORTED), (np.r_[col, 3], R.ST_BAD_BATCH),
                     (np.r_[-1, col], R.ST_BAD_BATCH), (np.r_[col[:10], 0.5, col[10:]], R.ST_BAD_BATCH | R.ST_UNSORTED)):
        for dtype in (F32, np.int32):
            if dtype is np.int32 and bit & R.ST_UNSORTED and bit & R.ST_BAD_BATCH:
                continue                                                    # 0.5 is no int32
            arr = np.asarray(bad, dtype)
            (cnt, start), st = with_status(ops.counts, cu(arr), 3)
            want_cnt, want_start, want_st = R.counts(arr, 3)
            assert st == want_st == bit, (bad, dtype)
            assert np.array_equal(cnt.cpu().numpy(), want_cnt) and np.array_equal(start.cpu().numpy(), want_start)
    (cnt, start), st = with_status(ops.counts, cu(np.zeros(0, F32)), 2)     # no rows at all
    assert st == 0 and cnt.cpu().tolist() == [0, 0] and start.cpu().tolist() == [0, 0, 0]


# ---- farthest point sampling ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fps_case(big):
    per = R.FPS_BIG_COUNTS if big else R.FPS_COUNTS
    xyz, start = R.stacked_cloud(2600 + len(per), per)
    return per, xyz, start, R.fps(xyz, start, R.FPS_K)


@pytest.mark.parametrize("big", [False, True], ids=["onchip", "scratch"])
def test_fps_equals_the_batched_op_per_sample_and_the_restatement(big):
    from dfu3d_amd import point_stack_ops as ops, pointnet2_ops as pn2
    per, xyz, start, (want_idx, want_kp, want_st) = fps_case(big)
    assert (sum(per) > ops.FPS_ONCHIP) == big and want_st == 0
    K = R.FPS_K
    (idx, kp), st = with_status(ops.fps, cu(xyz), cu(start), K)
    idx, kp = idx.cpu().numpy(), kp.cpu().numpy()
    assert st == 0 and idx.dtype == np.int32 and idx.shape == (len(per), K) and kp.shape == (len(per) * K, 4)
    assert np.array_equal(idx, want_idx) and np.array_equal(bits(kp), bits(want_kp))
    for b, n in enumerate(per):
        lo = int(start[b])
        alone, alone_xyz = pn2.fps(cu(xyz[None, lo:lo + n]), min(n, K))
        alone = alone.cpu().numpy()[0]
        assert np.array_equal(idx[b, :min(n, K)], alone)
        assert np.array_equal(idx[b], alone[np.arange(K) % len(alone)])     # a short sample cycles its picks
        assert np.array_equal(kp[b * K:(b + 1) * K, 1:], xyz[lo + idx[b]]) and (kp[b * K:(b + 1) * K, 0] == b).all()
    # in place from columns 1..3 of a wider block; a cap that changes the kernel's shape; twice: the same bits
    block = np.concatenate([np.zeros((len(xyz), 1), F32), xyz, np.ones((len(xyz), 2), F32)], axis=1)
    (idx2, kp2), st2 = with_status(ops.fps, cu(block)[:, 1:4], cu(start), K, cap=max(per))
    assert st2 == 0 and np.array_equal(idx2.cpu().numpy(), idx) and np.array_equal(bits(kp2.cpu().numpy()), bits(kp))


def test_fps_zero_count_and_cap_set_their_bits():
    from dfu3d_amd import point_stack_ops as ops
    per = [50, 0, 9]
    xyz, start = R.stacked_cloud(11, per)
    want_idx, want_kp, want_st = R.fps(xyz, start, 12)
    (idx, kp), st = with_status(ops.fps, cu(xyz), cu(start), 12)
    assert st == want_st == R.ST_EMPTY
    assert np.array_equal(idx.cpu().numpy(), want_idx) and np.array_equal(bits(kp.cpu().numpy()), bits(want_kp))
    assert not idx[1].any().item() and kp[12:24].cpu().tolist() == [[1.0, 0.0, 0.0, 0.0]] * 12
    (idx, kp), st = with_status(ops.fps, cu(xyz), cu(start), 12, cap=20)    # sample 0 is beyond the cap
    assert st == R.ST_EMPTY | R.ST_BAD_COUNT and int(idx[0].max()) < 20
    (idx, kp), st = with_status(ops.fps, cu(xyz), cu(np.asarray([0, 70, 40, 59], np.int32)), 12)
    assert st & R.ST_BAD_COUNT and int(idx.max()) < 59                       # starts beyond the rows: clamped


# ---- ball query, grouping ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def grid_case():
    """Points and centres on a 0.25 grid, all samples in the same region (they overlap in space); sample 5 is dense
    (more hits than any nsample), some centres lie far outside (empty balls)."""
    rng = np.random.default_rng(42)
    xyz = (rng.integers(-3, 4, (sum(R.BALL_N), 3)) * 0.25).astype(F32)
    ctr = (rng.integers(-3, 4, (sum(R.BALL_M), 3)) * 0.25).astype(F32)
    ctr[::7] += F32(40.0)                                                    # nothing near them
    return xyz, R.starts(R.BALL_N), ctr, R.starts(R.BALL_M)


@functools.lru_cache(maxsize=None)
def ball_ref(radius, nsample):
    xyz, start, ctr, cstart = grid_case()
    return R.ball_query(xyz, start, ctr, cstart, radius, nsample)


@pytest.mark.parametrize("nsample", R.BALL_NSAMPLE)
def test_ball_query_matches_the_restatement(nsample):
    from dfu3d_amd import point_stack_ops as ops
    xyz, start, ctr, cstart = grid_case()
    r = 0.5
    d2 = R.sqdist(ctr[:, None, :], xyz[None, :, :])
    assert (d2 == F32(r) * F32(r)).any()                                     # points exactly on the sphere exist
    want_idx, want_empty = ball_ref(r, nsample)
    assert want_empty.any() and not want_empty.all()
    dense = slice(int(cstart[5]), int(cstart[6]))
    assert ((d2[dense, int(start[5]):] < F32(0.25)).sum(1) > nsample).any()   # the walk exits early somewhere
    args = (cu(xyz), cu(start), cu(ctr), cu(cstart))
    ((idx, empty),), st = with_status(ops.ball_query, *args, [r], [nsample])
    assert st == 0
    idx, empty = idx.cpu().numpy(), empty.cpu().numpy()
    assert idx.shape == (len(ctr), nsample) and empty.dtype == np.uint8
    assert np.array_equal(idx, want_idx) and np.array_equal(empty, want_empty)
    for b in range(len(R.BALL_N)):                                           # only the centre's own sample
        rows = idx[int(cstart[b]):int(cstart[b + 1])]
        assert rows.size == 0 or rows.max() < max(R.BALL_N[b], 1)
    assert not idx[empty == 1].any()
    # two scales in one launch equal the scales alone; twice: the same bits
    other = 16 if nsample != 16 else 4
    both, st = with_status(ops.ball_query, *args, [r, 1.0], [nsample, other])
    assert st == 0 and np.array_equal(both[0][0].cpu().numpy(), idx) and np.array_equal(both[0][1].cpu().numpy(), empty)
    w1 = ball_ref(1.0, other)
    assert np.array_equal(both[1][0].cpu().numpy(), w1[0]) and np.array_equal(both[1][1].cpu().numpy(), w1[1])
    again = ops.ball_query(*args, [r, 1.0], [nsample, other])
    assert all(np.array_equal(a.cpu().numpy(), b.cpu().numpy()) for pa, pb in zip(both, again) for a, b in zip(pa, pb))


def test_ball_query_reads_columns_in_place():
    from dfu3d_amd import point_stack_ops as ops
    xyz, start, ctr, cstart = grid_case()
    pts = np.concatenate([np.full((len(xyz), 1), 9, F32), xyz, np.full((len(xyz), 1), 7, F32)], axis=1)
    kps = np.concatenate([np.full((len(ctr), 1), 9, F32), ctr], axis=1)
    ((idx, empty),) = ops.ball_query(cu(pts)[:, 1:4], cu(start), cu(kps)[:, 1:4], cu(cstart), [0.5], [16])
    want = ball_ref(0.5, 16)
    assert np.array_equal(idx.cpu().numpy(), want[0]) and np.array_equal(empty.cpu().numpy(), want[1])


@pytest.mark.parametrize("C", R.GROUP_C)
def test_group_layout_bits_and_empty_balls(C):
    from dfu3d_amd import point_stack_ops as ops
    xyz, start, ctr, cstart = grid_case()
    idx, empty = ball_ref(0.5, 16)
    feat = None
    if C:
        raw = np.random.default_rng(C).integers(0, 2 ** 32, (len(xyz), C), dtype=np.uint64).astype(np.uint32)
        raw[::3] |= 0x7FC00000                                               # NaNs with payloads among them
        feat = raw.view(F32)
    want = R.group(xyz, start, ctr, cstart, feat, idx, empty)
    out, st = with_status(ops.group, cu(xyz), cu(start), cu(ctr), cu(cstart), None if feat is None else cu(feat),
                          cu(idx), cu(empty))
    out = out.cpu().numpy()
    assert st == 0 and out.shape == (3 + C, len(ctr), 16)
    assert np.array_equal(bits(out), bits(want))
    assert not bits(out)[:, empty == 1].any()


def test_plain_grouping_operation_and_the_reference_names():
    """pointnet2_stack_utils under the reference's signatures: ball_query's mask, grouping_operation (features only,
    (M, C, nsample)) with its gradient, QueryAndGroup."""
    import torch
    from dfu3d_amd.pcdet_kitti import pointnet2_stack_utils as U
    xyz, start, ctr, cstart = grid_case()
    want_idx, want_empty = ball_ref(0.5, 16)
    cnt, ccnt = cu(np.asarray(R.BALL_N, np.int32)), cu(np.asarray(R.BALL_M, np.int32))
    idx, mask = U.ball_query(0.5, 16, cu(xyz), cnt, cu(ctr), ccnt)
    assert mask.dtype == torch.bool and np.array_equal(idx.cpu().numpy(), want_idx)
    assert np.array_equal(mask.cpu().numpy(), want_empty.astype(bool))
    feat = np.random.default_rng(12).normal(size=(len(xyz), 6)).astype(F32)
    # an index of a sample without points (sample 0) is outside its sample: zeros forward, left out of the backward
    own = np.repeat(np.asarray(R.BALL_N), R.BALL_M) > 0
    no_rows = (~own).astype(np.uint8)
    want = R.group(xyz, start, ctr, cstart, feat, want_idx, no_rows)[3:].transpose(1, 0, 2)
    f = cu(feat).requires_grad_(True)
    out = U.grouping_operation(f, cnt, idx, ccnt)
    assert tuple(out.shape) == (len(ctr), 6, 16) and np.array_equal(bits(out.detach().cpu().numpy()), bits(want))
    grad = np.random.default_rng(13).normal(size=want.shape).astype(F32)
    out.backward(cu(grad))
    padded = np.concatenate([np.zeros((3,) + grad.transpose(1, 0, 2).shape[1:], F32), grad.transpose(1, 0, 2)])
    want_grad = R.group_backward(padded, start, cstart, want_idx, no_rows, len(xyz))
    assert np.array_equal(bits(f.grad.cpu().numpy()), bits(want_grad))
    grouper = U.QueryAndGroup(0.5, 16, use_xyz=True)
    both, again = grouper(cu(xyz), cnt, cu(ctr), ccnt, cu(feat))
    assert np.array_equal(again.cpu().numpy(), want_idx)
    assert np.array_equal(bits(both.cpu().numpy()), bits(R.group(xyz, start, ctr, cstart, feat, want_idx, want_empty)))


def test_group_bad_index_sets_its_bit_and_stays_inside():
    from dfu3d_amd import point_stack_ops as ops
    xyz, start, ctr, cstart = grid_case()
    idx, empty = ball_ref(0.5, 16)
    bad = idx.copy()
    m = int(np.nonzero(empty == 0)[0][-1])
    bad[m, 3] = 10 ** 6
    feat = np.random.default_rng(3).normal(size=(len(xyz), 4)).astype(F32)
    out, st = with_status(ops.group, cu(xyz), cu(start), cu(ctr), cu(cstart), cu(feat), cu(bad), cu(empty))
    fixed = idx.copy()
    fixed[m, 3] = 0
    assert st == R.ST_BAD_INDEX
    assert np.array_equal(bits(out.cpu().numpy()), bits(R.group(xyz, start, ctr, cstart, feat, fixed, empty)))


def test_group_backward_ordered_sum():
    import torch
    from dfu3d_amd import point_stack_ops as ops
    xyz, start, ctr, cstart = grid_case()
    idx, empty = ball_ref(1.0, 32)
    N, C = len(xyz), 5
    hits = np.bincount((idx + np.repeat(start[:-1], R.BALL_M)[:, None])[empty == 0].ravel().astype(np.int64), minlength=N)
    assert hits.max() > 32 and (hits == 0).any() and empty.any()            # a row in many balls, a row in none
    rng = np.random.default_rng(8)
    feat = rng.normal(size=(N, C)).astype(F32)
    grad = (rng.normal(size=(3 + C, len(ctr), 32)) * 10.0 ** rng.integers(-3, 4, (3 + C, len(ctr), 32))).astype(F32)
    want = R.group_backward(grad, start, cstart, idx, empty, N)
    args = (cu(xyz), cu(start), cu(ctr), cu(cstart))
    got = []
    for _ in range(2):
        f = cu(feat).requires_grad_(True)
        st = torch.zeros(1, dtype=torch.int32, device='cuda')
        with ops.status_scope(st):
            out = ops.query_group(*args, f, cu(idx), cu(empty))
            out.backward(cu(grad))
        assert int(st.item()) == 0                                           # the left-out entries raise nothing
        assert f.grad.shape == (N, C)
        got.append(f.grad.cpu().numpy())
    assert np.array_equal(bits(got[0]), bits(want)) and np.array_equal(bits(got[0]), bits(got[1]))
    assert not bits(got[0])[hits == 0].any()                                 # +0.0, not -0.0
    # a genuinely bad index is reported by the stage's own kernel, and left out
    bad = idx.copy()
    m = int(np.nonzero(empty == 0)[0][0])
    bad[m, 0] = -5
    gf, st = with_status(ops.group_backward, cu(grad), cu(bad), cu(empty), cu(start), cu(cstart), N)
    assert st == R.ST_BAD_INDEX


# ---- bilinear BEV sampling -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [3, 70])
def test_bev_sample_matches_the_restatement(C):
    from dfu3d_amd import point_stack_ops as ops
    B, H, W = 2, 5, 7
    rng = np.random.default_rng(C)
    spatial = rng.normal(size=(B, C, H, W)).astype(F32)
    pc_range, voxel, stride = [-1.4, -1.0, -1.0], [0.1, 0.1, 0.2], 2       # one cell of the map is 0.2 m
    xy = rng.uniform([-1.4, -1.0], [0.0, 0.0], (40, 2))
    edges = [[-5.0, -0.5], [5.0, -0.5], [-0.7, -5.0], [-0.7, 5.0], [-5.0, -5.0], [5.0, 5.0], [-1.41, -1.01], [0.0, 0.0]]
    whole = [[-1.4 + 0.2 * i, -1.0 + 0.2 * j] for i in range(W) for j in range(H)]   # integer map coordinates
    xy = np.concatenate([xy, edges, whole]).astype(F32)
    kp = np.concatenate([rng.integers(0, B, (len(xy), 1)).astype(F32), xy, rng.normal(size=(len(xy), 1)).astype(F32)], 1)
    want = R.bev_sample(kp, spatial, pc_range, voxel, stride)
    fx = ((kp[:, 1] - F32(pc_range[0])) / F32(voxel[0])) / F32(stride)
    assert (fx == np.floor(fx)).sum() >= 5 and (fx < 0).any() and (fx > W).any()
    out, st = with_status(ops.bev_sample, cu(kp), cu(spatial), pc_range, voxel, stride)
    assert st == 0 and np.array_equal(bits(out.cpu().numpy()), bits(want))
    kp[3, 0] = B                                                             # a sample that does not exist: zeros
    out, st = with_status(ops.bev_sample, cu(kp), cu(spatial), pc_range, voxel, stride)
    assert st == R.ST_BAD_BATCH and not out[3].any().item()
