"""The planted inputs of tests/fuse_cases.py have the properties they are there for -- checked on the CPU with the oracle
and the kernel's cell arithmetic as tests/fuse_cases.py restates it: which cell a neighbour lies in, which LiDAR points
are outside the quantised range, how long a chain is and which cells share a slot, what the radius filter leaves of a
LiDAR list, that both outcomes occur right at the threshold, and that no statistical-filter input sits on a knife edge
of its threshold."""
import math

import numpy as np
import pytest

from oracle import penet_oracle as O
from tests import fuse_cases as F

PLAIN = F.plain_cases()
BY = {c.name: c for c in PLAIN}


def _keep(case, s):
    a, b = case.A[s], case.B[s]
    return O.ball_query(b, a, case.C) if len(a) and len(b) else np.ones(len(b), bool)


# ------------------------------------------------------------------------------------------------ the restated arithmetic
def test_restated_cell_arithmetic():
    for C in F.THRESHOLD_CS:
        u = F.unit(C)
        assert u == C * (1.0 + 1e-5) / 16.0
        x = np.array([0.0, 0.5 * u, -0.5 * u, 31.5 * u, 32.5 * u, -4092.0 * C, 4091.0 * C])
        assert F.quant(x, C).tolist()[:5] == [65536.0, 65536.0, 65535.0, 65567.0, 65568.0]
        assert (F.quant(x[:5], C).astype(np.int64) >> 5).tolist() == [2048, 2048, 2047, 2048, 2049]
        # the range: [64, 131000) quantised, about +-4092 C
        assert F.in_range(np.array([[4091.0 * C, 0, 0], [-4091.9 * C, 0, 0]]), C).all()
        assert not F.in_range(np.array([[4092.0 * C, 0, 0], [0, -4092.1 * C, 0], [0, 0, np.nan], [np.inf, 0, 0], [5000.0 * C, 0, 0]]), C).any()
    assert 409.1 < (F.Q_HI - F.OFF) * F.unit(0.1) < 409.2 and -409.3 < (F.Q_LO - F.OFF) * F.unit(0.1) < -409.2
    assert [F.table_slots(n) for n in (1, 128, 129, 1024, 1025, 4096)] == [256, 256, 512, 2048, 4096, 8192]
    assert (F.SMALL_TILE, F.BIG_TILE) == (341, 1365)
    assert F.bh_hash(0, 0, 0) == 0 and F.bh_hash(1, 0, 0) == 0x9E3779 ^ (0x9E3779 >> 15) ^ ((0x9E3779 ^ (0x9E3779 >> 15)) >> 7)
    # a mid-cell query walks one cell per axis, an off-centre one two
    W = 32 * F.unit(0.1)
    assert len(F.candidate_cells(np.array([0.5 * W] * 3), 0.1)) == 1
    assert len(F.candidate_cells(np.array([0.25 * W] * 3), 0.1)) == 8


# ------------------------------------------------------------------------------------------------ every plain case
@pytest.mark.parametrize("case", PLAIN, ids=[c.name for c in PLAIN])
def test_range_and_outcome_mix(case):
    """The LiDAR lists named as fallback have a point outside [64, 131000), the others have none; every case has at least
    20 kept and 20 dropped queries, or exactly the one outcome it is named for."""
    kept = dropped = 0
    for s, a in enumerate(case.A):
        outside = int((~F.in_range(a, case.C)).sum())
        assert (outside >= 1) == case.fallback[s], (case.name, s, outside)
        k = _keep(case, s)
        kept += int(k.sum())
        dropped += int((~k).sum())
    if case.expect == "all":
        assert dropped == 0 and kept >= 20
    elif case.expect == "none":
        assert kept == 0 and dropped >= 20
    else:
        assert kept >= 20 and dropped >= 20, (case.name, kept, dropped)


@pytest.mark.parametrize("C", F.THRESHOLD_CS)
def test_threshold_pairs_are_isolated_and_fall_on_both_sides(C):
    case = BY["threshold_C%g" % C]
    assert case.info["pitch"] >= 1.0
    kept = dropped = 0
    for s, (a, b) in enumerate(zip(case.A, case.B)):
        for q in b:
            d = F.dist(q, a)
            assert int((d < 3.0 * C).sum()) == 1, s                       # exactly one candidate
            assert abs(d.min() / C - 1.0) < 2e-5                           # and that one at C (1 +- rel)
        k = _keep(case, s)
        kept += int(k.sum())
        dropped += int((~k).sum())
        lim = 4092.0 * C
        assert (np.abs(a) < lim).all() or case.fallback[s]
    assert kept >= 20 and dropped >= 20, (C, kept, dropped)
    # the centres: the origin, +-40 m and +-400 m (scaled with C), negative coordinates among them
    m = np.array([np.abs(a).max() for a in case.A[:6]]) / (C / 0.1)
    assert m[0] < 10 and 35 < m[1] < 50 and 35 < m[2] < 50 and (m[3:] > 395).all() and (m[3:] < 409).all()
    assert case.A[2].max() < 0 and case.A[4].max() < 0
    # the undecidable pairs (rel at or below the rounding of the coordinates) fall on both sides
    far = case.A[3], case.B[3]
    d = np.array([F.dist(q, far[0]).min() for q in far[1]])
    tight = np.abs(d / C - 1.0) < 1e-11
    kt = O.ball_query(far[1][tight], far[0], C)
    assert kt.sum() >= 5 and (~kt).sum() >= 5


@pytest.mark.parametrize("C", F.THRESHOLD_CS)
def test_phase_sweep_reaches_the_top_of_the_pruning_bound(C):
    """Every query is kept, has one candidate, and the quantised bound of its pair takes values over the whole span that
    a neighbour at C (1 - 1e-9) = 15.9998 units can produce: 225 along an axis (a difference of 16 units), 200 / 221 / 242
    on a face diagonal (two differences of 11 or 12), 192 / 209 / 226 / 243 on the body diagonal (three of 9 or 10), all of
    them <= 257."""
    case = BY["phase_C%g" % C]
    a, b = case.A[0], case.B[0]
    assert _keep(case, 0).all()
    sums = []
    for q in b:
        d = F.dist(q, a)
        assert int((d < 3.0 * C).sum()) == 1
        sums.append(F.prune_sum(a[d.argmin()], q, C))
    sums = np.array(sums)
    assert sums.max() <= F.PRUNE_BOUND
    assert set(sums.tolist()) == {225.0, 200.0, 221.0, 242.0, 192.0, 209.0, 226.0, 243.0}, sorted(set(sums.tolist()))
    assert (sums > 225).sum() >= 20                      # pairs a bound of 225 would prune
    # every phase k / 64 of a unit occurs on every axis
    ph = np.floor((a / F.unit(C) - np.floor(a / F.unit(C))) * 64.0).astype(int)
    for ax in range(3):
        assert set(ph[:, ax].tolist()) == set(range(64))


def test_border_neighbours_sit_in_the_stated_adjacent_cell():
    case = BY["borders"]
    C, a, b = case.C, case.A[0], case.B[0]
    assert F.in_range(a, C).all()
    keep = _keep(case, 0)
    seen = set()
    Cq, u = C * (1.0 + 1e-6), F.unit(C)
    for qi, ai, delta, kind in case.info["queries"]:
        q = b[qi]
        d = F.dist(q, a)
        cq, cn = F.cell_of(q[None], C)[0], F.cell_of(a[ai][None], C)[0]
        assert tuple(cn - cq) == delta, (qi, delta)
        if kind == "far":
            assert (d < C).sum() == 0 and d.argmin() == ai and d[ai] < 1.1 * C
        else:
            assert (d < C).sum() == 1 and d.argmin() == ai               # no other LiDAR point within C
        if kind == "reach":                                              # the neighbour's cell is entered by less than 0.1 C
            ax = int(np.abs(a[ai] - q).argmax())
            edge = q[ax] + Cq * delta[ax]
            border = ((cn[ax] + (delta[ax] < 0)) * 32 - F.OFF) * u
            assert delta[ax] != 0 and 0 < (edge - border) * delta[ax] < 0.1 * C and 0.9 * C < d[ai] < C
        assert bool(keep[qi]) == (kind != "far")
        # the eight cells of the walk -- the query's own among them -- all hold a LiDAR point farther than C
        cells = F.candidate_cells(q, C)
        assert len(cells) == 8 and tuple(cq) in cells and tuple(cn) in cells
        ca = F.cell_of(a, C)
        for cell in cells:
            inside = (ca == np.array(cell)).all(1)
            assert (d[inside] > C).any(), (qi, cell)
        seen.add((delta, kind))
    assert len(seen) == 3 * 26                                           # one, two and three axes, low and high side
    assert sorted({sum(1 for x in dl if x) for dl, _ in seen}) == [1, 2, 3]


def test_dense_cell_and_shared_slots():
    case = BY["dense"]
    C, a, b = case.C, case.A[0], case.B[0]
    ca = F.cell_of(a, C)
    in_cell = (ca == np.array(case.info["cell"])).all(1)
    assert in_cell.sum() >= 200 and in_cell.all()                        # one chain of 262 nodes
    kind = case.info["kind"]
    walks = 0
    for q, k in zip(b, kind):
        near = np.nonzero(F.dist(q, a) < C)[0]
        if k == "tail":
            assert near.tolist() == [0]
        elif k == "head":
            assert near.tolist() == [len(a) - 1]
        elif k == "none":
            assert len(near) == 0
        else:
            assert len(near) > 5
        through = tuple(case.info["cell"]) in F.candidate_cells(q, C)    # the walk goes through the dense cell
        assert through or k == "none"
        walks += int(through and k == "none")
    assert walks >= 20                                                   # also for queries that find nothing at its end
    assert {k: int((kind == k).sum()) for k in ("tail", "head", "none", "inside")} == dict(tail=30, head=30, none=50, inside=30)

    case = BY["shared_slots"]
    a = case.A[0]
    assert len(a) == 1024 and F.in_range(a, case.C).all()
    cells = np.unique(F.cell_of(a, case.C), axis=0)
    slots = F.slot_of_cells(cells, len(a))
    per_slot = np.bincount(slots, minlength=F.table_slots(len(a)))
    assert F.table_slots(len(a)) == 2048 and len(cells) > 1000
    assert (per_slot >= 2).sum() >= 50 and per_slot.max() >= 3           # several occupied cells in one slot
    # and queries whose neighbour is reached through such a slot
    keep = _keep(case, 0)
    shared = 0
    for q in case.B[0][keep][:200]:
        j = int(F.dist(q, a).argmin())
        shared += int(per_slot[F.slot_of_cells(F.cell_of(a[j][None], case.C), len(a))[0]] >= 2)
    assert shared >= 20


def test_boundary_counts_and_patterns():
    case = BY["boundaries"]
    na = [len(a) for a in case.A]
    nb = [len(b) for b in case.B]
    assert set(na) >= {1, 2, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097}
    small = {n for m, n in zip(na, nb) if m <= F.SMALL_MAX}
    big = {n for m, n in zip(na, nb) if F.SMALL_MAX < m <= F.BIG_MAX}
    brute = {n for m, n in zip(na, nb) if m > F.BIG_MAX}
    assert small >= {255, 256, 257} and big >= {1023, 1024, 1025, 2049} and brute >= {1023, 1024, 1025, 2049}
    assert small >= {F.SMALL_BT - 1, F.SMALL_BT, F.SMALL_BT + 1}         # around the query tile of either build
    assert big >= {F.BIG_BT - 1, F.BIG_BT, F.BIG_BT + 1, 2 * F.BIG_BT + 1} and brute >= {F.BIG_BT - 1, F.BIG_BT, F.BIG_BT + 1}
    assert set(na) >= {F.SMALL_MAX, F.SMALL_MAX + 1, F.BIG_MAX, F.BIG_MAX + 1}     # the last list of a class, the first of the next
    assert {2047, 2048, 2049, 4097} <= {n for (_, n, p) in F.BOUNDARY_INSTANCES if p == "alt"}
    for s, (m, n, pat) in enumerate(F.BOUNDARY_INSTANCES):
        assert (na[s], nb[s]) == (m, n)
        keep = _keep(case, s)
        assert np.array_equal(keep, case.info["patterns"][s]), s         # the planted pattern is what the oracle decides
        if pat == "all":
            assert keep.all()
        elif pat == "none":
            assert not keep.any()
        elif pat == "alt" and n > F.COMPACT_STEP:                        # the pattern flips at the step of the compaction
            i = np.arange(n)
            assert np.array_equal(keep[:F.COMPACT_STEP], (i[:F.COMPACT_STEP] // 3) % 2 == 0)
            assert np.array_equal(keep[F.COMPACT_STEP:2 * F.COMPACT_STEP], (i[F.COMPACT_STEP:2 * F.COMPACT_STEP] // 3) % 2 == 1)
    for want in ("all", "none"):                                          # in all three classes
        cls = {0 if m <= F.SMALL_MAX else 1 if m <= F.BIG_MAX else 2 for (m, _, p) in F.BOUNDARY_INSTANCES if p == want}
        assert cls == {0, 1, 2}


def test_fallback_instances():
    case = BY["fallback"]
    C = case.C
    assert [len(a) for a in case.A[:8]] == [1, 341, 342, 683, 1024, 1366, 2731, 4096]
    for s in range(8):
        a, b = case.A[s], case.B[s]
        out = np.nonzero(~F.in_range(a, C))[0]
        assert len(out) == 1 and a[out[0], 0] == 500.0                   # one LiDAR point at 500 m
        keep = _keep(case, s)
        assert keep[-1] and F.dist(b[-1], a).argmin() == out[0]          # a query beyond the range that is kept by it
        assert not F.in_range(b[-1:], C)[0]
        if len(a) == 1:
            continue
        tile = F.SMALL_TILE if len(a) <= F.SMALL_MAX else F.BIG_TILE
        t0 = ((len(a) - 1) // tile) * tile
        lt = case.info["last_tile"][s]
        assert len(lt) >= 1 and (lt >= t0).all() and out[0] not in lt
        for q in b[:40]:                                                 # neighbours in the last tile only
            near = np.nonzero(F.dist(q, a) < C)[0]
            assert len(near) >= 1 and (near >= t0).all()
        assert keep[:40].all()
    # all points near 500 m
    a, b = case.A[8], case.B[8]
    assert not F.in_range(a, C).any() and not F.in_range(b, C).any() and a.min() > 490.0
    # queries beyond the range next to LiDAR points just inside it: the table path
    a, b = case.A[9], case.B[9]
    assert F.in_range(a, C).all() and not case.fallback[9]
    assert not F.in_range(b, C).any()
    keep = _keep(case, 9)
    assert keep[:120].sum() >= 20 and (~keep[:120]).sum() >= 20 and not keep[120:].any()
    f = F.quant(b, C)
    assert ((f > F.Q_MAX).any(1) | (f < 0).any(1)).sum() >= 30           # some beyond all 17 bits, on either side
    assert (f > F.Q_MAX).any() and (f < 0).any()


def test_nonfinite_instances():
    case = BY["nonfinite"]
    assert [len(a) for a in case.A] == [300, 2000, 4200, 300, 2000, 4200]
    for s, (a, b) in enumerate(zip(case.A, case.B)):
        bad = case.info["bad_q"][s]
        assert np.array_equal(bad, ~np.isfinite(b).all(1)) and bad.sum() == 11
        assert np.isnan(b[bad]).any() and np.isposinf(b[bad]).any() and np.isneginf(b[bad]).any()
        keep = _keep(case, s)
        assert not keep[bad].any()                                       # the oracle drops them
        assert keep[~bad].sum() >= 20 and (~keep[~bad]).sum() >= 20     # the rest of the list decides as usual
        assert (~np.isfinite(a).all(1)).sum() == (0, 0, 0, 1, 1, 2)[s]
    assert np.isnan(case.A[3]).any() and np.isposinf(case.A[4]).any()
    assert np.isnan(case.A[5]).any() and np.isneginf(case.A[5]).any()


def test_joint_case_is_what_the_filter_makes_of_it():
    j = F.joint_case()
    assert [len(a) for a in j.A] == [502, 4200, 4200, 1024]
    # 0: the far pair survives the filter and is outside the range
    k0 = O.radius_outlier(j.A[0], 1, j.ra[0])
    pair = j.info["pair"]
    assert len(pair) == 2 and set(pair.tolist()) <= set(k0.tolist())
    assert not F.in_range(j.A[0][pair], 0.1).any() and (j.A[0][pair][:, 0] >= 600.0).all()
    assert abs(F.dist(j.A[0][pair[0]], j.A[0][pair[1:]])[0] - 0.3) < 1e-9
    assert F.in_range(np.delete(j.A[0], pair, 0), 0.1).all()
    # 1: the whole first brute-force tile goes, later points stay
    k1 = O.radius_outlier(j.A[1], 1, j.ra[1])
    assert len(j.A[1]) > F.BIG_MAX and k1.min() >= j.info["n_isolated"] > F.BIG_TILE and len(k1) > 2000
    # 2, 3: nothing is left
    assert len(O.radius_outlier(j.A[2], 1, j.ra[2])) == 0 and len(O.radius_outlier(j.A[3], 1, j.ra[3])) == 0
    assert len(j.A[3]) == F.SMALL_MAX
    # every instance has pseudo points left after their filter, so 2 and 3 count as skipped fuses
    for s in range(4):
        assert len(O.radius_outlier(j.B[s], 1, j.rb[s])) >= 50
    # and the fuse decides both ways where it runs
    for s in (0, 1):
        a1 = j.A[s][O.radius_outlier(j.A[s], 1, j.ra[s])]
        b1 = j.B[s][O.radius_outlier(j.B[s], 1, j.rb[s])]
        k = O.ball_query(b1, a1, 0.1)
        assert k.sum() >= 20 and (~k).sum() >= 20
    # the pseudo points next to the far pair are kept by it alone
    b1 = j.B[0][O.radius_outlier(j.B[0], 1, j.rb[0])]
    assert (O.ball_query(b1, j.A[0][pair], 0.1)).sum() >= 5


# ------------------------------------------------------------------------------------------------ statistical filter
def _stat_margin(pts, k, ratio):
    """min over the points with a positive mean distance of |v - thr| / |thr| (inf where nothing depends on thr)."""
    v = O.knn_mean_dist(pts, k)
    n = len(v)
    mu = 0.0
    for x in v:
        mu += x if x > 0 else 0.0
    mu /= n
    sq = 0.0
    for x in v:
        sq += (x - mu) * (x - mu) if x > 0 else 0.0
    thr = mu + ratio * math.sqrt(sq / (n - 1))
    pos = v[v > 0]
    if len(pos) == 0 or thr == 0.0:
        return math.inf, v, thr
    return float(np.abs(pos - thr).min() / abs(thr)), v, thr


@pytest.mark.parametrize("k", F.STAT_KS)
def test_no_statistical_threshold_on_a_knife_edge(k):
    """The kernel sums the mean distances in another order than the oracle, so mu and with it the threshold may differ in
    the last bits: every enabled segment must have min |v_i - thr| > 1e-9 |thr| over its points with v_i > 0 (v_i = 0 --
    nb_neighbors = 1, duplicates -- is decided by v > 0 alone).  Two structural exceptions, in which the threshold is the
    same on both sides whatever the order of the sums: n = 1 (the deviation is NaN, nothing is kept) and n = 2 (both
    mean distances are the same number v, so mu = (v + v) / 2 = v and the deviation 0 exactly)."""
    segs, enable = F.stat_segments()
    assert sorted(len(s) for s, e in zip(segs, enable) if e) == sorted(F.STAT_SIZES)
    assert {0, 1, 2, 3, 127, 128, 129, 1023, 1024, 1025, 2100} <= set(F.STAT_SIZES)
    assert {F.KNN_QT - 1, F.KNN_QT, F.KNN_QT + 1, F.KNN_PT - 1, F.KNN_PT, F.KNN_PT + 1, 2 * F.KNN_PT + 52} <= set(F.STAT_SIZES)
    assert max(F.STAT_KS) == F.KNN_MAX
    assert set(F.STAT_KS) == {1, 2, 5, 30, 63, 64} and set(F.STAT_RATIOS) == {-1.0, 0.0, 0.3, 2.0, 1e9}
    assert any(0 < len(s) < k for s, e in zip(segs, enable) if e) or k == 1          # a count larger than the segment
    assert list(enable) == [1, 0] * len(F.STAT_SIZES)
    for ratio in F.STAT_RATIOS:
        for s, (pts, e) in enumerate(zip(segs, enable)):
            if not e or len(pts) == 0:
                continue
            if len(pts) == 1:
                assert len(O.statistical_outlier(pts, k, ratio)) == 0
                continue
            margin, v, thr = _stat_margin(pts, k, ratio)
            if len(pts) == 2:
                assert v[0] == v[1] and len(O.statistical_outlier(pts, k, ratio)) == (2 if v[0] > 0 and thr > v[0] else 0)
                assert ratio > 0 or thr <= v[0]
                if ratio > 0 and v[0] > 0:
                    assert thr == v[0]                               # deviation 0: thr = mu = v, v < thr is false
                continue
            assert margin > 1e-9, (k, ratio, s, len(pts), margin)
            if k == 1:
                assert not v.any() and len(O.statistical_outlier(pts, k, ratio)) == 0
            if ratio == 1e9 and k > 1:
                assert len(O.statistical_outlier(pts, k, ratio)) == int((v > 0).sum()) == len(pts)


def test_duplicate_segments():
    segs, enable, where = F.duplicate_segments()
    assert list(enable) == [1, 1, 0]
    assert len(segs[0]) == 40 and (segs[0] == segs[0][0]).all()
    assert not O.knn_mean_dist(segs[0], 30).any() and len(O.statistical_outlier(segs[0], 30, 0.3)) == 0
    v = O.knn_mean_dist(segs[1], 30)
    assert len(where) == 35 and not v[where].any() and (np.delete(v, where) > 0).all()
    for ratio in (0.3, 2.0):
        keep = O.statistical_outlier(segs[1], 30, ratio)
        assert not set(keep.tolist()) & set(where.tolist()) and 20 <= len(keep) <= 300 - 35 - (20 if ratio < 1 else 1)
        margin, _, _ = _stat_margin(segs[1], 30, ratio)
        assert margin > 1e-9
