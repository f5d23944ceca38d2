"""dfu3d_ballquery_fuse (plain, masked, joint) and dfu3d_stat_filter on the inputs at which segment_stage.hip takes another
path, against the CPU oracle: pairs at distance C (1 +- 1e-5 ... 0) for three values of C, every phase of the quantised
pruning bound, neighbours only across a cell border, chains of hundreds of nodes and shared hash slots, LiDAR counts on
the edges of the two table builds and the brute-force tiles, pseudo counts around the query tiles and the compaction
step, the fallback from the table to brute force (a LiDAR point beyond the quantised range, non-finite LiDAR points),
non-finite queries, LiDAR lists the radius filter empties in part or whole; for the statistical filter segment sizes
around the 128-query and the 1024-point tile, nb_neighbors 1 .. 64, five values of std_ratio, duplicates, and the
per-point mean distances themselves.  The inputs are planted in tests/fuse_cases.py (their properties are checked on
the CPU by tests/test_fuse_cases_host.py).  Every comparison is exact: kept sets, counts, the updated bases, the
surviving coordinates bit for bit in list order, everything outside the lists untouched, mean distances bit for bit."""
import numpy as np
import pytest
import torch

from oracle import penet_oracle as O
from tests import fuse_cases as F
from tests.fit_cases import pool_from_segments
from tests.test_gpu_radius_filter import _joint_filter_then_fuse_equals_oracle
from tests.test_gpu_stages import _ballquery_fuse_run, _masked_fuse_verify, _stat_filter_run, _stat_filter_verify

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
PLAIN = F.plain_cases()


@pytest.fixture(scope="module")
def st():
    from dfu3d_amd import stages
    return stages


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(got, exp):
    return got.shape == exp.shape and np.array_equal(_bits(got), _bits(exp))


# ------------------------------------------------------------------------------------------------ ball query
@pytest.mark.parametrize("case", PLAIN, ids=[c.name for c in PLAIN])
def test_ballquery_fuse_case(st, case):
    """One dfu3d_ballquery_fuse call per case of tests/fuse_cases.py, every instance against O.ball_query."""
    base_a, ncb, nbase, X = _ballquery_fuse_run(st, case.A, case.B, C=case.C)
    total = sum(len(a) + len(b) for a, b in zip(case.A, case.B))
    kept = dropped = 0
    for s, (a, b) in enumerate(zip(case.A, case.B)):
        keep = O.ball_query(b, a, case.C) if len(a) and len(b) else np.ones(len(b), bool)
        kept += int(keep.sum())
        dropped += int((~keep).sum())
        got = X[nbase[s]:nbase[s] + ncb[s]]
        assert ncb[s] == keep.sum(), (case.name, s, int(ncb[s]), int(keep.sum()),
                                      "first difference at query %s" % _first_difference(got, b, keep))
        assert nbase[s] == base_a[s] + len(a), (case.name, s)
        exp = np.concatenate([a, b[keep]])                              # A directly followed by the kept B, bit for bit
        assert _same_bits(X[base_a[s]:base_a[s] + len(exp)], exp), (case.name, s, _first_difference(got, b, keep))
    assert X.shape[0] == total + 16 and (X[total:] == 9.0).all()       # nothing behind the lists was touched
    if case.expect == "mix":
        assert kept >= 20 and dropped >= 20


def _first_difference(got, b, keep):
    """Index in b of the first query whose outcome differs from the oracle's (for the message of a failure)."""
    exp = b[keep]
    n = min(len(got), len(exp))
    neq = np.nonzero((_bits(got[:n]) != _bits(exp[:n])).any(1))[0]
    k = int(neq[0]) if len(neq) else n
    idx = np.nonzero(keep)[0]
    return int(idx[k]) if k < len(idx) else None


def test_masked_fuse_over_the_fallback_instances(st):
    """The fallback instances once more behind the radius filter of the pseudo lists (dfu3d_ballquery_fuse_masked): a
    radius that keeps every pseudo point and one that drops most of them, in turn."""
    case = next(c for c in PLAIN if c.name == "fallback")
    radius = np.array([3.0, 0.3] * len(case.A))[:len(case.A)]
    base_a, ncb, _, X = _ballquery_fuse_run(st, case.A, case.B, radius=radius, C=case.C)
    _masked_fuse_verify(case.A, case.B, radius, base_a, ncb, X)
    left = [len(O.radius_outlier(b, 1, r)) for b, r in zip(case.B, radius)]
    assert min(left[0::2]) >= 250 and 0 < max(left[1::2]) < 250        # both kinds of mask were there


def test_joint_fuse_with_lists_the_filter_empties(st):
    """The far LiDAR pair that survives the filter (fallback under the LiDAR mask), a first brute-force tile that the filter
    empties, a brute-force list and a table it empties whole (fuse skipped, every filtered pseudo point stays)."""
    j = F.joint_case()
    skipped = _joint_filter_then_fuse_equals_oracle(st, j.A, j.B, j.ra, j.rb)
    assert skipped >= 2


# ------------------------------------------------------------------------------------------------ statistical filter
SENTINEL = -7.25


def _stat_run(st, segs, enable, k, ratio, raises=None):
    """One dfu3d_stat_filter call over the padded pool of pool_from_segments -> dict of what went in and came out.
    raises: the call must fail with this error (match "dfu3d_stat_filter")."""
    P, base, cnt, cap = pool_from_segments(segs)
    px, py, pz = _t(P[:, 0]), _t(P[:, 1]), _t(P[:, 2])
    S = len(segs)
    seg_cnt = _t(cnt)
    tile_off = torch.zeros(S + 1, dtype=torch.int32, device=DEV)
    flags = torch.zeros(cap, dtype=torch.uint8, device=DEV)
    mean_d = torch.full((cap,), SENTINEL, dtype=torch.float64, device=DEV)
    args = (px, py, pz, _t(base), seg_cnt, _t(enable), k, ratio, S, cap, tile_off, flags, mean_d)
    if raises is None:
        st.stat_filter(*args)
    else:
        with pytest.raises(raises, match="dfu3d_stat_filter"):
            st.stat_filter(*args)
    torch.cuda.synchronize()
    return dict(P=P, base=base, cnt=cnt, cap=cap, out=seg_cnt.cpu().numpy(), X=torch.stack([px, py, pz], 1).cpu().numpy(),
                mean_d=mean_d.cpu().numpy(), flags=flags.cpu().numpy())


_KNN = {}


def _knn(key, pts, k):
    """O.knn_mean_dist, computed once per (segment, k) and shared by the tests; read-only."""
    if (key, k) not in _KNN:
        v = O.knn_mean_dist(pts, k)
        v.setflags(write=False)
        _KNN[key, k] = v
    return _KNN[key, k]


def _stat_verify(r, tag, segs, enable, k, ratio):
    base, out, X, P = r["base"], r["out"], r["X"], r["P"]
    outside = np.ones(r["cap"], bool)
    for s, pts in enumerate(segs):
        n = len(pts)
        outside[base[s]:base[s] + n] = False
        if not enable[s]:
            assert out[s] == n and _same_bits(X[base[s]:base[s] + n], pts), (tag, s, "a disabled segment changed")
            continue
        if n == 0:
            assert out[s] == 0
            continue
        md = r["mean_d"][base[s]:base[s] + n]
        exp_md = _knn((tag, s), pts, k)
        assert np.array_equal(_bits(md), _bits(exp_md)), (tag, s, n, k, "mean distances differ at",
                                                          np.nonzero(_bits(md) != _bits(exp_md))[0][:5])
        keep = O.statistical_outlier(pts, k, ratio)
        assert out[s] == len(keep), (tag, s, n, k, ratio, int(out[s]), len(keep))
        assert _same_bits(X[base[s]:base[s] + out[s]], pts[keep]), (tag, s, n, k, ratio)
    assert _same_bits(X[outside], P[outside])                          # pads and the pool behind the lists untouched
    assert (r["mean_d"][outside] == SENTINEL).all()


@pytest.mark.parametrize("k", F.STAT_KS)
def test_stat_filter_sizes_neighbours_and_ratios(st, k):
    """Sizes 0 .. 2100 around the 128-query and the 1024-point tile, each next to a disabled segment, for every std_ratio;
    nb_neighbors = 1 makes every mean distance 0 (all dropped); 20- and smaller segments have fewer points than neighbours
    are asked for.  The mean distances are compared bit for bit with O.knn_mean_dist."""
    segs, enable = F.stat_segments()
    for ratio in F.STAT_RATIOS:
        r = _stat_run(st, segs, enable, k, ratio)
        _stat_verify(r, "sizes", segs, enable, k, ratio)
        if k == 1:
            assert not r["out"][enable == 1].any()
        if ratio == 1e9 and k > 1:
            # keeps every point whose mean distance is positive -- from three points on: one point has no deviation (NaN), and
            # the two mean distances of a pair are the same number, so their deviation is 0 and v < mu + 1e9 * 0 is false
            assert [int(c) for c in r["out"][enable == 1]] == [n if n >= 3 else 0 for n in F.STAT_SIZES]
    # the runner and the checker of tests/test_gpu_stages.py, on the same segments
    base, out, X = _stat_filter_run(st, segs, enable, k, 0.3)
    _stat_filter_verify(segs, enable, k, 0.3, base, out, X)


def test_stat_filter_duplicates(st):
    """40 copies of one point: every mean distance is 0, all dropped.  35 copies inside a clustered segment: those are
    dropped, the rest is judged as usual."""
    segs, enable, where = F.duplicate_segments()
    for ratio in (0.3, 2.0):
        r = _stat_run(st, segs, enable, 30, ratio)
        _stat_verify(r, "dup", segs, enable, 30, ratio)
        assert r["out"][0] == 0 and 20 <= r["out"][1] <= 300 - 35
        md = r["mean_d"][r["base"][1]:r["base"][1] + 300]
        assert not md[where].any() and (np.delete(md, where) > 0).all()


@pytest.mark.parametrize("k", [0, 65, -3])
def test_stat_filter_refuses_a_neighbour_count_out_of_range(st, k):
    """nb_neighbors below 1 or above 64: the library's error, and nothing is written."""
    segs, enable = F.stat_segments()
    r = _stat_run(st, segs, enable, k, 0.3, raises=st.Dfu3dError)
    assert _same_bits(r["X"], r["P"]) and np.array_equal(r["out"], r["cnt"])
    assert (r["mean_d"] == SENTINEL).all() and not r["flags"].any()
