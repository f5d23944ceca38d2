"""The fit stage (dfu3d_range_cluster + dfu3d_lshape_fit) on the sizes at which fit_stage.hip takes another path, against
the CPU oracle: cluster sizes around the three fit kernels, the LDS chunk and the scheduling rounds; segments in every
launch class; more than 512 / 1 024 clusters in one instance (passes of k_fit_gather, whose own contract on sx / sy /
sroot is checked directly); links that only the farther point's radius makes; the three forms of the point-level
fallback; heading counts up to the table's last entry, with and without ties between headings; row and descriptor
overflow.  The instances are planted in tests/fit_cases.py (their properties are checked on the CPU by
tests/test_fit_cases_host.py); integers, memberships, member counts, roots and heading indices must be equal, fp64
geometry within 1e-9, all 24 row columns compared."""
import numpy as np
import pytest
import torch

from oracle import penet_oracle as O
from tests import fit_cases as F

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENTINEL = -12345.678


@pytest.fixture(scope="module")
def st():
    from dfu3d_amd import stages
    return stages


def _t(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV).contiguous()


def _oracle_calib(c):
    return O.Calibration({"P2": c.P2, "R0": c.R0, "Tr_velo2cam": c.V2C})


class _Instances:
    """Segments (x, y of the cases + a seeded z), padded to whole views of M instances; class, 2D box and score distinct
    per instance, every second one flagged is_car, one calibration per view (three yaw angles in turn)."""

    def __init__(self, xys, M, seed):
        from dfu3d_amd import synth
        rng = np.random.default_rng(seed)
        self.M = M
        self.segs = [np.concatenate([np.asarray(xy, np.float64).reshape(-1, 2), rng.uniform(-1.7, 0.3, (len(xy), 1))], 1)
                     for xy in xys]
        while len(self.segs) % M:
            self.segs.append(np.zeros((0, 3)))
        self.S = len(self.segs)
        self.V = self.S // M
        self.classes = [(3 * i + 1) % 10 for i in range(self.S)]
        self.iscar = [i % 2 for i in range(self.S)]
        self.boxes = [[100.0 + i, 50.5 + 2 * i, 300.25 + 3 * i, 200.0 + 5 * i] for i in range(self.S)]
        self.scores = [0.05 + 0.9 * ((7 * i + 3) % self.S) / self.S for i in range(self.S)]
        self.cals = [synth.make_calibration((30.0, -55.0, 110.0)[v % 3], 900, 1600, rng) for v in range(self.V)]
        self.ocals = [_oracle_calib(c) for c in self.cals]

    def expected(self, oparams):
        return F.expected_rows(self.segs, self.M, self.classes, self.iscar, self.boxes, self.scores, self.ocals, oparams)


class _Run:
    pass


def _fit(st, inst, n_theta, dtheta, cap_rows, R0=3.0, Rd=0.001, car_aspect_max=5.0, fit_ws=None, pool=None):
    """dfu3d_range_cluster + dfu3d_lshape_fit on the instances.  `rows` is a slice out of the middle of a larger
    allocation filled with a sentinel.  pool: the tensors of an earlier run on the same instances (clustering reused)."""
    r = _Run()
    if pool is None:
        P, base, cnt, cap = F.pool_from_segments(inst.segs)
        r.base, r.cnt, r.cap = base, cnt, cap
        r.px, r.py, r.pz = _t(P[:, 0]), _t(P[:, 1]), _t(P[:, 2])
        r.tb, r.tc = _t(base), _t(cnt)
        r.label = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
        st.range_cluster(r.px, r.py, r.tb, r.tc, inst.S, R0, Rd, r.label, cap)
    else:
        for k in ("base", "cnt", "cap", "px", "py", "pz", "tb", "tc", "label"):
            setattr(r, k, getattr(pool, k))
    cap = r.cap
    guard = 64 * st.ROW_DOUBLES
    r.arena = torch.full((2 * guard + cap_rows * st.ROW_DOUBLES,), SENTINEL, dtype=torch.float64, device=DEV)
    r.rows = r.arena[guard:guard + cap_rows * st.ROW_DOUBLES]
    r.n_rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    r.status = torch.zeros(1, dtype=torch.int32, device=DEV)
    r.sx = torch.full((cap,), SENTINEL, dtype=torch.float64, device=DEV)
    r.sy = torch.full((cap,), SENTINEL, dtype=torch.float64, device=DEV)
    r.sroot = torch.full((cap,), -9, dtype=torch.int32, device=DEV)
    st.lshape_fit(r.px, r.py, r.pz, r.label, r.tb, r.tc, inst.S, inst.M, _t(np.stack([c.record() for c in inst.cals])),
                  _t(np.array(inst.classes, np.int32)), _t(np.array(inst.iscar, np.int32)),
                  _t(np.array(inst.boxes, np.float32)), _t(np.array(inst.scores, np.float32)), n_theta, dtheta,
                  car_aspect_max, r.sx, r.sy, r.sroot, cap_rows, r.rows, r.n_rows, r.status, cap, fit_ws=fit_ws)
    torch.cuda.synchronize()
    r.n = int(r.n_rows.item())
    r.st = int(r.status.item())
    a = r.arena.cpu().numpy()
    r.guards_intact = bool((a[:guard] == SENTINEL).all() and (a[guard + cap_rows * st.ROW_DOUBLES:] == SENTINEL).all())
    r.R = a[guard:guard + cap_rows * st.ROW_DOUBLES].reshape(cap_rows, st.ROW_DOUBLES)
    return r


def _thetas(dtheta_deg=1.0):
    from dfu3d_amd.params import Params
    return Params(dtheta_deg=dtheta_deg).thetas()


def _check_labels(r, inst, labels):
    """labels: the oracle's, per segment (second result of expected_rows)."""
    lab = r.label.cpu().numpy()
    for s, pts in enumerate(inst.segs):
        assert (labels[s] >= 0).all() and np.array_equal(lab[r.base[s]:r.base[s] + len(pts)], labels[s]), s
    return lab


# ------------------------------------------------------------------------------------------------ (a) cluster-size edges
def test_cluster_sizes_on_the_edges_of_the_fit_kernels(st):
    """One single-cluster instance per member count 64 | 65 (k_fit_tiny | k_fit_medium), 2 048 | 2 049 (members in LDS |
    the big list), 4 096 | 4 097 and 8 192 | 8 193 (staging chunks of k_fit_big_cost), 6 144 | 6 145 (its scheduling
    rounds; 8 193 points is also launch class 1 of the gather): three views with a calibration each."""
    cases = F.edge_size_cases()
    inst = _Instances([c.pts for c in cases], 4, 21)
    assert inst.V == 3
    n_theta, dtheta = _thetas()
    r = _fit(st, inst, n_theta, dtheta, 64)
    assert r.st == 0 and r.guards_intact
    exp, labels = inst.expected(O.Params())
    _check_labels(r, inst, labels)
    assert sorted(exp[:, 17].astype(int).tolist()) == sorted(F.EDGE_SIZES) and r.n == len(exp)
    F.assert_rows_match(r.R[:r.n], exp, dtheta)


# ------------------------------------------------------------------------------------------------ (b) long clusters / segments
def test_long_clusters_and_long_segments(st):
    """A cluster of 16 385 members (round 0 of k_fit_big_cost, five staging chunks) and an instance of 16 696 points with
    clusters of 16 384, 300 and 1 member interleaved (launch class 0 of the gather; the last size of round 1), short
    and empty instances between them."""
    one, mixed = F.long_cases()
    rng = np.random.default_rng(22)
    short = F.lshape(rng, 9.0, -6.0, 4.4, 1.8, 0.2, 90)
    pair = np.array([[5.0, 5.0], [5.5, 6.0]])
    inst = _Instances([one.pts, short, np.zeros((0, 2)), pair, mixed.pts, np.zeros((0, 2))], 4, 23)
    n_theta, dtheta = _thetas()
    r = _fit(st, inst, n_theta, dtheta, 128)
    assert r.st == 0 and r.guards_intact
    exp, labels = inst.expected(O.Params())
    _check_labels(r, inst, labels)
    assert r.n == len(exp) >= 16
    F.assert_rows_match(r.R[:r.n], exp, dtheta)


# ------------------------------------------------------------------------------------------------ (c) + (f) many clusters
@pytest.fixture(scope="module")
def many():
    """The instance of 533 clusters, one of 1 056 singletons and a short one in one view; the expected rows once."""
    rng = np.random.default_rng(24)
    inst = _Instances([F.many_cluster_case().pts, F.singleton_case().pts, F.lshape(rng, 9.0, -6.0, 4.4, 1.8, 0.2, 90)], 4, 25)
    exp, labels = inst.expected(O.Params())
    exp.setflags(write=False)
    return inst, exp, labels


def test_more_than_512_clusters_in_one_instance(st, many):
    """Two and three passes of k_fit_gather's counting sort (512 clusters each): every row, and the gather's own
    contract -- sroot holds the instance's roots in ascending order, sx / sy hold the clusters in that order, each
    cluster's members contiguous and in index order."""
    inst, exp, labels = many
    n_theta, dtheta = _thetas()
    r = _fit(st, inst, n_theta, dtheta, 2048)
    assert r.st == 0 and r.guards_intact
    lab = _check_labels(r, inst, labels)
    assert r.n == len(exp) == 533 + 1056 + 1
    F.assert_rows_match(r.R[:r.n], exp, dtheta)
    sx, sy, sroot = r.sx.cpu().numpy(), r.sy.cpu().numpy(), r.sroot.cpu().numpy()
    for s, pts in enumerate(inst.segs):
        b, n = int(r.base[s]), len(pts)
        L = lab[b:b + n]
        roots = np.unique(L)
        assert np.array_equal(sroot[b:b + len(roots)], roots), s
        order = np.lexsort((np.arange(n), L))              # by cluster (= by root), members in index order
        assert np.array_equal(sx[b:b + n], pts[order, 0]) and np.array_equal(sy[b:b + n], pts[order, 1]), s


def test_row_and_descriptor_overflow(st, many):
    """cap_rows = 8 (80 cluster descriptors) against 1 590 clusters: the status word says so, the eight rows written
    are eight different rows of the full set, nothing is written outside rows[0 : cap_rows] -- and the same call with
    room (same workspace tensor) then returns status 0 and the full set: the workspace header is zeroed per call."""
    inst, exp, _ = many
    n_theta, dtheta = _thetas()
    roomy = 2048
    pool_cap = F.pool_from_segments(inst.segs)[3]
    ws = torch.zeros(int(st._lib.lib().dfu3d_lshape_fit_ws_doubles(pool_cap, roomy)), dtype=torch.float64, device=DEV)
    r = _fit(st, inst, n_theta, dtheta, 8, fit_ws=ws)
    assert r.st & st.ST_ROW_OVERFLOW and r.n >= 8
    assert r.guards_intact
    by_key = {tuple(int(v) for v in e[:3]): e for e in exp}
    seen = set()
    for g in r.R:
        key = tuple(int(v) for v in g[:3])
        assert key in by_key and key not in seen, key
        seen.add(key)
        F.assert_row_matches(g, by_key[key], dtheta)
    r2 = _fit(st, inst, n_theta, dtheta, roomy, fit_ws=ws, pool=r)
    assert r2.st == 0 and r2.guards_intact and r2.n == len(exp)
    F.assert_rows_match(r2.R[:r2.n], exp, dtheta)


# ------------------------------------------------------------------------------------------------ (d) clustering
def _cluster(st, cases, R0, Rd):
    segs = [np.concatenate([c, np.zeros((len(c), 1))], 1) for c in cases]
    P, base, cnt, cap = F.pool_from_segments(segs)
    label = torch.full((cap,), -7, dtype=torch.int32, device=DEV)
    st.range_cluster(_t(P[:, 0]), _t(P[:, 1]), _t(base), _t(cnt), len(segs), R0, Rd, label, cap)
    torch.cuda.synchronize()
    lab = label.cpu().numpy()
    return [lab[base[s]:base[s] + len(c)] for s, c in enumerate(cases)]


@pytest.mark.parametrize("family", ["far", "near"])
def test_links_through_the_farther_points_radius_only(st, family):
    """Two dense blobs whose only link is one pair with R_i < d <= R_j, d stepped across R_j in the last ulps on either
    side.  far: Rd = 0.05 at 30 m, no grid variant is eligible, the fallback's point-level rule decides; near: the twin at
    Rd = 0.001 around the origin, on the grid path."""
    cases = F.asym_far_cases() if family == "far" else F.asym_near_cases()
    R0, Rd = cases[0].R0, cases[0].Rd
    got = _cluster(st, [c.pts for c in cases], R0, Rd)
    outcomes = set()
    for c, lab in zip(cases, got):
        exp = O.range_cluster_labels(c.pts[:, 0], c.pts[:, 1], R0, Rd)
        assert np.array_equal(lab, exp), c.name
        outcomes.add(len(np.unique(exp)))
    assert outcomes == {1, 2}


@pytest.mark.parametrize("n", F.FALLBACK_SIZES)
def test_fallback_forms(st, n):
    """Instances wider than the largest grid: 32-bit parents in LDS up to 4 096 points, 16-bit parents up to 61 440,
    parents in global memory beyond."""
    c = F.fallback_case(n)
    got, = _cluster(st, [c.pts], c.R0, c.Rd)
    assert np.array_equal(got, O.range_cluster_labels(c.pts[:, 0], c.pts[:, 1], c.R0, c.Rd))
    assert np.bincount(got)[np.unique(got)].tolist() == c.sizes


# ------------------------------------------------------------------------------------------------ (e) heading counts
@pytest.mark.parametrize("dtheta_deg,n_expected", [(2.0, 44), (1.0, 89), (0.75, 119), (0.7, 128)])
def test_heading_counts(st, dtheta_deg, n_expected):
    """An even count below 64 (k_fit_tiny's second heading per lane is skipped), an odd one, a partial batch of 16 and
    the last entry of the heading table, one cluster per fit kernel."""
    n_theta, dtheta = _thetas(dtheta_deg)
    assert n_theta == n_expected
    rng = np.random.default_rng(26)
    inst = _Instances([F.lshape(rng, 12.0, 3.0, 4.6, 1.9, 0.4, 40), F.lshape(rng, -20.0, 8.0, 7.0, 2.5, 1.2, 500),
                       F.lshape(rng, 15.0, -9.0, 4.4, 1.8, -0.9, 5000)], 4, 27)
    r = _fit(st, inst, n_theta, dtheta, 16)
    assert r.st == 0 and r.guards_intact
    exp, labels = inst.expected(O.Params(dtheta_deg=dtheta_deg))
    _check_labels(r, inst, labels)
    assert r.n == len(exp) == 3
    F.assert_rows_match(r.R[:r.n], exp, dtheta)


@pytest.mark.parametrize("dtheta_deg,n_expected", F.TIE_HEADINGS)
def test_heading_ties_on_the_size_edges_at_every_heading_count(st, dtheta_deg, n_expected):
    """Point sets invariant under turns of 6 degrees (F.ring_tie_cases: 14 or 15 headings within the band at 44, 89 and
    119 headings, two at 128, indices of 64 and more among them -- tests/test_fit_cases_host.py) with exactly 64 | 65,
    2 048 | 2 049 and 4 097 members: tier 2, the band rule and the three-sweep cost in every fit kernel, in the second
    heading slot of a lane of k_fit_tiny and in a second staging chunk of k_fit_big_cost.  The reference's arg-max as an
    index, all 24 columns.  Six of the twenty (case, heading count) are left out: there the library and numpy land on
    different members of the tied set (F.TIE_DISAGREE has the indices)."""
    cases = F.ring_tie_cases_at(n_expected)
    inst = _Instances([c.pts for c in cases], 4, 31)
    n_theta, dtheta = _thetas(dtheta_deg)
    assert n_theta == n_expected
    r = _fit(st, inst, n_theta, dtheta, 16)
    assert r.st == 0 and r.guards_intact
    exp, labels = inst.expected(O.Params(dtheta_deg=dtheta_deg))
    _check_labels(r, inst, labels)
    assert exp[:, 17].astype(int).tolist() == [c.n for c in cases] and r.n == len(exp)
    F.assert_rows_match(r.R[:r.n], exp, dtheta)


def test_more_headings_than_the_table_holds_are_refused(st):
    """n_theta = 129 > MAXTH: DFU3D_ERANGE before anything is launched -- rows, n_rows and status stay as they were."""
    from dfu3d_amd._lib import Dfu3dError
    rng = np.random.default_rng(28)
    inst = _Instances([F.lshape(rng, 12.0, 3.0, 4.6, 1.9, 0.4, 40)], 4, 29)
    P, base, cnt, cap = F.pool_from_segments(inst.segs)
    rows = torch.full((16 * st.ROW_DOUBLES,), SENTINEL, dtype=torch.float64, device=DEV)
    n_rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    z = lambda dt: torch.zeros(cap, dtype=dt, device=DEV)
    with pytest.raises(Dfu3dError):
        st.lshape_fit(_t(P[:, 0]), _t(P[:, 1]), _t(P[:, 2]), z(torch.int32), _t(base), _t(cnt), inst.S, inst.M,
                      _t(np.stack([c.record() for c in inst.cals])), _t(np.array(inst.classes, np.int32)),
                      _t(np.array(inst.iscar, np.int32)), _t(np.array(inst.boxes, np.float32)),
                      _t(np.array(inst.scores, np.float32)), 129, 0.0122, 5.0, z(torch.float64), z(torch.float64),
                      z(torch.int32), 16, rows, n_rows, status, cap)
    torch.cuda.synchronize()
    assert int(n_rows.item()) == 0 and int(status.item()) == 0 and bool((rows == SENTINEL).all())
