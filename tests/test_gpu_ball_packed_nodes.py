"""dfu3d_ballquery_fuse where the packed node test of k_ball_flags (cell-local bytes, one dot product, bound 314) could go
wrong: pairs whose quantised differences sit on the bound, queries at both ends of q - 32 u, hash slots shared with a
foreign node whose bytes look like a neighbour's, chains of 300 nodes walked to the end, the LiDAR counts at which the
build changes, the ends of the quantised range, and the masked modes.  Expected flags come from the oracle's distances
(fuse_cases.dist); every comparison is exact.  The inputs are built once per module and small."""
import numpy as np
import pytest

from tests import ball_packed as P
from tests import fuse_cases as F
from tests.test_gpu_radius_filter import _joint_filter_then_fuse_equals_oracle
from tests.test_gpu_stages import _ballquery_fuse_run, _masked_fuse_verify

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def st():
    from dfu3d_amd import stages
    return stages


def _check(st, A, B, C):
    """One dfu3d_ballquery_fuse call; every instance's kept pseudo points against the oracle's distances.
    -> per instance the keep mask."""
    A = [np.ascontiguousarray(a, np.float64).reshape(-1, 3) for a in A]
    B = [np.ascontiguousarray(b, np.float64).reshape(-1, 3) for b in B]
    base_a, ncb, nbase, X = _ballquery_fuse_run(st, A, B, C=C)
    keeps = []
    for s, (a, b) in enumerate(zip(A, B)):
        keep = P.keep_by_oracle_distance(a, b, C)
        got = X[nbase[s]:nbase[s] + ncb[s]]
        exp = b[keep]
        same = got.shape == exp.shape and np.array_equal(got.view(np.uint64), exp.view(np.uint64))
        if not same:
            n = min(len(got), len(exp))
            bad = np.nonzero((got[:n].view(np.uint64) != exp[:n].view(np.uint64)).any(1))[0]
            raise AssertionError("instance %d: %d kept, %d expected, first difference at kept position %s"
                                 % (s, len(got), len(exp), int(bad[0]) if len(bad) else n))
        assert nbase[s] == base_a[s] + len(a)
        assert np.array_equal(X[base_a[s]:base_a[s] + len(a)].view(np.uint64), a.view(np.uint64))
        keeps.append(keep)
    return keeps


# ------------------------------------------------------------------------------------------------ bound phases
def _triples():
    """Non-negative sorted triples of quantised differences with their sum of squares and the parent's prune sum."""
    out = []
    for a in range(0, 19):
        for b in range(a, 19):
            for c in range(b, 19):
                d = np.array([a, b, c])
                out.append((d, int((d * d).sum()), int(P.old_prune_sum(d))))
    return out


def _plant_pairs(rng, C, wanted, site0):
    """For every (signed difference triple D, distance in units r or None): a LiDAR point and a query whose quantised
    coordinates differ by exactly D; with r the pair is r units apart, otherwise somewhere in the triple's range.
    Found by sampling the point's phase inside its unit and the direction; triples that cannot be met are left out.
    -> (A, B, D of the pairs that were planted)."""
    u = F.unit(C)
    pitch = 64.0                                       # units between pairs: two cells
    A, B, Ds = [], [], []
    for k, (D, r) in enumerate(wanted):
        D = np.asarray(D, np.int64)
        n = 20000
        ph = rng.uniform(0.0, 1.0, (n, 3))
        t = D[None, :] - ph + rng.uniform(0.0, 1.0, (n, 3))          # floor(ph + t) = D
        if r is not None:
            t *= (r / np.linalg.norm(t, axis=1))[:, None]
        ok = np.nonzero((np.floor(ph + t) == D[None, :]).all(1))[0]
        site = (np.array([k % 12, (k // 12) % 12, k // 144]) + site0) * pitch + rng.integers(0, 32, 3)
        for i in ok[:8]:
            a = (site + ph[i]) * u
            q = a + t[i] * u
            if r is not None:                                        # the distance exactly as asked, in metres
                q = a + (q - a) * (r * u / np.linalg.norm(q - a))
            if np.array_equal(F.quant(q, C) - F.quant(a, C), D.astype(np.float64)):
                A.append(a); B.append(q); Ds.append(D)
                break
    return np.array(A), np.array(B), np.array(Ds)


BOUND_RELS = (1e-9, 1e-15)


@pytest.fixture(scope="module")
def bound_cases():
    """Per C: (A, B, D).  Pairs at distance C (1 -+ rel) with the largest sums of squares a neighbour can have, and pairs
    whose differences give sum d^2 = 313, 314, 315 or the parent's prune sum 257, 258 (all of them farther than C: a
    neighbour's prune sum is below 256)."""
    out = {}
    tr = _triples()
    for C in F.THRESHOLD_CS:
        rng = np.random.default_rng(6300 + int(C * 1000))
        units_C = C / F.unit(C)
        near = sorted([t for t in tr if t[2] < 250 and ((t[0] + 1) ** 2).sum() > 260], key=lambda t: -t[1])[:24]
        on_bound = [t for t in tr if t[1] in (313, 314, 315) or t[2] in (257, 258)]
        wanted = []
        for d, _, _ in near:
            for rel in BOUND_RELS:
                for sign in (-1.0, 1.0):
                    perm = rng.permutation(3)
                    wanted.append((d[perm] * rng.choice([-1, 1], 3), units_C * (1.0 + sign * rel)))
        for d, _, _ in on_bound:
            for _ in range(2):
                perm = rng.permutation(3)
                wanted.append((d[perm] * rng.choice([-1, 1], 3), None))
        out[C] = _plant_pairs(rng, C, wanted, site0=np.array([-6, 3, 1]))
    return out


@pytest.mark.parametrize("C", F.THRESHOLD_CS)
def test_pairs_on_the_bound(st, bound_cases, C):
    A, B, D = bound_cases[C]
    d2, prune = (D * D).sum(1), P.old_prune_sum(D)
    for v in (313, 314, 315):
        assert (d2 == v).sum() >= 2, v                                     # the phases were planted
    for v in (257, 258):
        assert (prune == v).sum() >= 2, v
    p = np.random.default_rng(1).permutation(len(B))
    keep = _check(st, [A], [B[p]], C)[0]
    assert keep.sum() >= 20 and (~keep).sum() >= 20
    assert d2[p][keep].max() >= 290                                         # neighbours close to the bound were kept
    assert not keep[(prune[p] >= 257)].any()


# ------------------------------------------------------------------------------------------------ range ends
def test_queries_at_both_ends_of_the_cell_offset(st):
    """Queries whose quantised coordinate sits 15 or 16 units into its cell on one axis: q - 32 u reaches 47 for the low
    cell of the walk and -16 for the high one (the values rounding allows; the kernel admits -17 .. 48).  The only
    LiDAR point within C lies across that border, 0.97 C away (or just behind the border where that is farther); for
    every other query it is 1.03 C away."""
    C = 0.1
    rng = np.random.default_rng(6400)
    u = F.unit(C)
    A, B = [], []
    k = 0
    for ax in range(3):
        for m, side in ((15, -1.0), (16, 1.0)):
            for frac in (0.01, 0.5, 0.99):
                for dist_rel in (0.97, 1.03):
                    cell = np.array([2048 + 3 * (k % 7) - 9, 2048 - 3 * ((k // 7) % 7) + 5, 2048 + 3 * (k // 49)])
                    k += 1
                    loc = rng.choice([8.0, 24.0], 3) + rng.uniform(0.1, 0.9, 3)
                    loc[ax] = m + frac
                    q = (cell * 32.0 + loc - F.OFF) * u
                    a = q.copy()
                    to_border = (m + frac if side < 0 else 32.0 - (m + frac)) * u      # 15.01 .. 15.99 units, C is 15.9998
                    a[ax] += side * max(dist_rel * C, to_border + 0.004 * u)
                    A.append(a); B.append(q)
    A, B = np.array(A), np.array(B)
    r_lo, r_hi = [], []
    for ax in range(3):
        q, x0, x1, qin = P.walk_of(B[:, ax], C)
        assert qin.all()
        r_lo.append(q - 32 * x1); r_hi.append(q - 32 * x0)
    assert np.min(r_lo) == -16 and np.max(r_hi) == 47
    assert (F.cell_of(A, C) != F.cell_of(B, C)).any(1).all()               # every neighbour across a border
    keep = _check(st, [A], [B], C)[0]
    assert keep.sum() == len(B) // 2


# ------------------------------------------------------------------------------------------------ shared slots
def test_foreign_nodes_in_a_shared_slot_are_not_kept_on_their_bytes(st):
    """Pairs of cells in ONE hash slot (planted with fuse_cases.slot_of_cells).  A query in the first cell; the second
    cell holds a LiDAR point at the same place inside its cell, so its bytes are the query's own: the packed sum is 0 and
    only the exact predicate rejects it.  Half of the queries also have a true neighbour in their own cell."""
    C = 0.1
    rng = np.random.default_rng(6500)
    u = F.unit(C)
    na = 200
    cells = np.stack(np.meshgrid(np.arange(2030, 2070), np.arange(2035, 2055), np.arange(2044, 2052), indexing="ij"), -1).reshape(-1, 3)
    slots = F.slot_of_cells(cells, na)
    A, B, expect, foreign_d2 = [], [], [], []
    used = set()
    for s in np.unique(slots):
        idx = np.nonzero(slots == s)[0]
        if len(idx) < 2 or len(B) >= 60:
            continue
        c0, c1 = cells[idx[0]], cells[idx[1]]
        if np.abs(c0 - c1).max() < 2 or any(np.abs(c0 - np.array(o)).max() < 2 or np.abs(c1 - np.array(o)).max() < 2 for o in used):
            continue
        used.update([tuple(c0), tuple(c1)])
        loc = rng.uniform(4.0, 28.0, 3)
        q = (c0 * 32.0 + loc - F.OFF) * u
        A.append((c1 * 32.0 + loc + rng.uniform(-0.4, 0.4, 3) - F.OFF) * u)
        with_own = len(B) % 2 == 0
        if with_own:
            A.append(q + F._unit_vec(rng) * 0.5 * C)
        B.append(q); expect.append(with_own)
        foreign_d2.append(int(P.packed_d2(P.node_bytes(F.quant(A[-2 if with_own else -1], C).astype(np.int64)[None]),
                                          P.query_bytes(F.quant(q, C).astype(np.int64)[None], c0[None]))[0]))
    assert len(B) >= 20 and len(A) <= na
    fill = F._lattice_sites(rng, na - len(A), 5.0 * C, (30.0, 30.0, 5.0))      # the table's size is that of 200 points
    A = np.concatenate([np.array(A), fill])
    assert F.table_slots(len(A)) == F.table_slots(na)
    assert max(foreign_d2) <= 3                                               # the foreign bytes pass the packed test
    keep = _check(st, [A], [np.array(B)], C)[0]
    assert np.array_equal(keep, np.array(expect))


# ------------------------------------------------------------------------------------------------ long chains
def test_chain_of_300_nodes_walked_to_its_end(st):
    """300 LiDAR points in the middle of ONE cell.  Queries in the neighbouring cells that reach into it and are farther
    than C from every point walk all of their chains to the end; queries inside the crowd are kept."""
    C = 0.1
    rng = np.random.default_rng(6600)
    u = F.unit(C)
    cell = np.array([2048 - 11, 2048 + 4, 2048 + 2])
    lo = (cell * 32.0 - F.OFF) * u
    A = lo + rng.uniform(0.3, 0.7, (300, 3)) * 32 * u
    none = []
    for k in range(120):
        loc = rng.uniform(9.0, 23.0, 3)
        ax = k % 3
        loc[ax] = rng.uniform(-10.0, -7.5) if (k // 3) % 2 else rng.uniform(39.5, 42.0)      # at least 17 units from the crowd
        none.append(lo + loc * u)
    inside = lo + rng.uniform(0.35, 0.65, (60, 3)) * 32 * u
    B = np.concatenate([np.array(none), inside])
    for q in none[:6]:
        assert tuple(cell) in F.candidate_cells(q, C)
    p = rng.permutation(len(B))
    keep = _check(st, [A], [B[p]], C)[0]
    assert np.array_equal(keep, (np.arange(len(B)) >= 120)[p])


# ------------------------------------------------------------------------------------------------ build edges
@pytest.mark.parametrize("counts", [(1, 0, 1024, 1025), (4096,), (4097,)], ids=["small", "big", "brute"])
def test_lidar_counts_at_the_edges_of_the_builds(st, counts):
    C = 0.1
    rng = np.random.default_rng(6700 + len(counts) + counts[0])
    A, B = [], []
    for na in counts:
        pattern = rng.random(300) < 0.5
        if na == 0:
            A.append(np.zeros((0, 3))); B.append(rng.uniform(-5, 5, (300, 3)))
            continue
        a, b = F._planted_lists(rng, na, pattern, rng.uniform(-40, 40, 3), C)
        A.append(a); B.append(b)
    keeps = _check(st, A, B, C)
    for na, keep in zip(counts, keeps):
        assert keep.all() if na == 0 else (keep.sum() >= 100 and (~keep).sum() >= 100)


# ------------------------------------------------------------------------------------------------ quantised-range ends
def test_ends_of_the_quantised_range(st):
    """Instance 0 (table path): LiDAR points just inside the range of the table build on either side, queries 0.6 C and
    1.3 C beyond them, queries far beyond all 17 bits, NaN and infinite queries.
    Instance 1: the same with one LiDAR point outside the range -- the brute-force fallback."""
    C = 0.1
    rng = np.random.default_rng(6800)
    u = F.unit(C)
    hi_edge, lo_edge = (F.Q_MAX + 1 - 20 - F.OFF) * u, (F.Q_LO - F.OFF) * u
    a, b = [], []
    for k in range(90):
        ax, side = k % 3, (k // 3) % 2
        p = rng.uniform(-100, 100, 3)
        p[ax] = hi_edge - rng.uniform(60.0, 70.0) * u if side else lo_edge + rng.uniform(0.05, 0.4) * C
        step = np.zeros(3)
        step[ax] = (1.0 if side else -1.0) * (0.6 if k % 2 else 1.3) * C
        a.append(p); b.append(p + step)
    a = np.array(a)
    assert F.in_range(a, C).all()
    for k in range(30):                                                  # far beyond all 17 bits
        p = rng.uniform(-100, 100, 3)
        p[k % 3] = (1.0 if k % 2 else -1.0) * rng.uniform(450.0, 5000.0)
        b.append(p)
    b = np.array(b)
    b[3] = np.nan
    b[7, 1] = np.nan
    b[11, 2] = np.inf
    b[15, 0] = -np.inf
    far = np.array([[5000.0, 1.0, 1.0]])
    A = [a, np.concatenate([a[:40], far, a[40:]])]
    assert not F.in_range(A[1], C).all()
    keeps = _check(st, A, [b, b.copy()], C)
    assert np.array_equal(keeps[0], keeps[1])
    assert keeps[0].sum() >= 40 and not keeps[0][[3, 7, 11, 15]].any() and not keeps[0][90:].any()


def test_queries_outside_the_17_bits_next_to_points_inside(st):
    """C = 0.5: the quantised range ends at about +-2048 m.  LiDAR points in range by the rule of the table build need
    f >= 64, so a query outside the 17 bits (f < 0) is at least 64 units from them: such queries walk cell 0 and test its
    nodes exactly, and none is kept; queries just inside the 17 bits (f in [0, 64)) take the packed test at the clamped
    end of the range."""
    C = 0.5
    rng = np.random.default_rng(6900)
    u = F.unit(C)
    a, b = [], []
    for k in range(60):
        ax = k % 3
        p = rng.uniform(-50, 50, 3)
        p[ax] = (F.Q_LO + rng.uniform(0.1, 3.0) - F.OFF) * u             # the first units of the range, cell 2
        q = p.copy()
        q[ax] = (rng.uniform(-30.0, 63.0) - F.OFF) * u                  # outside the 17 bits or in cells 0, 1
        a.append(p); b.append(q)
        b.append(p + F._unit_vec(rng) * 0.5 * C)                        # and a query the point keeps
    a, b = np.array(a), np.array(b)
    assert F.in_range(a, C).all()
    qf = F.quant(b, C)
    assert (qf < 0).any() and ((qf >= 0) & (qf < 32)).any()
    keep = _check(st, [a], [b], C)[0]
    assert keep[1::2].all() and 0 < keep[0::2].sum() < 30
    assert not keep[0::2][(qf[0::2] < 0).any(1)].any()


# ------------------------------------------------------------------------------------------------ masked modes
def _masked_lists(rng):
    """Three instances: an ordinary one, one whose LiDAR points are all isolated (the joint filter empties the list), and
    one with a dense cell."""
    C = 0.1
    A, B = [], []
    body = rng.normal(0, 1.0, (600, 3))
    b = rng.normal(0, 1.0, (800, 3))
    b[:400] = body[rng.integers(0, 600, 400)] + rng.normal(0, 0.06, (400, 3))
    A.append(body); B.append(b)
    iso = F._lattice_sites(rng, 300, 8.0, (0.0, 0.0, 0.0))
    b = rng.normal(0, 20.0, (500, 3))
    b[:150] = iso[rng.integers(0, 300, 150)] + rng.normal(0, 0.06, (150, 3))
    A.append(iso); B.append(b)
    crowd = np.array([5.0, 5.0, 1.0]) + rng.uniform(0.0, 1.5 * C, (300, 3))
    b = np.array([5.0, 5.0, 1.0]) + rng.uniform(-3 * C, 4.5 * C, (500, 3))
    A.append(crowd); B.append(b)
    return A, B


def test_masked_mode_1(st):
    """The radius filter of the pseudo lists without compaction, then dfu3d_ballquery_fuse_masked."""
    A, B = _masked_lists(np.random.default_rng(7000))
    radius = np.array([0.3, 3.0, 0.05])
    base_a, ncb, _, X = _ballquery_fuse_run(st, A, B, radius=radius)
    _masked_fuse_verify(A, B, radius, base_a, ncb, X)


def test_masked_mode_2_with_a_lidar_list_the_filter_emptied(st):
    """The joint filter over both lists, then the fuse under both masks: instance 1's LiDAR list is emptied whole, so its
    fuse is skipped and every filtered pseudo point stays."""
    A, B = _masked_lists(np.random.default_rng(7100))
    skipped = _joint_filter_then_fuse_equals_oracle(st, A, B, np.array([3.0, 3.0, 3.0]), np.array([0.3, 3.0, 0.05]))
    assert skipped >= 1
