"""Inputs of the fit-stage tests (tests/test_gpu_fit_edges.py, tests/test_gpu_stages.py, tests/test_fit_cases_host.py):
instances planted on the sizes at which fit_stage.hip takes another path -- cluster sizes around the three fit kernels,
the LDS chunk and the scheduling rounds, segment lengths in every launch class, more than 512 and more than 1024
clusters in one instance, link decisions that only the farther point's radius takes, instances no grid variant accepts.
Every builder returns the points TOGETHER WITH the properties the case is there for (FitCase); tests/test_fit_cases_host.py
checks those properties with the oracle, so an edit here cannot silently move a case off its path.  numpy only, seeded;
the expected rows (expected_rows) come from the oracle, none are stored."""
import math
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

ROW_COLS = 24                       # DFU3D_ROW_DOUBLES
EDGE_SIZES = (64, 65, 2048, 2049, 4096, 4097, 6144, 6145, 8192, 8193)
FALLBACK_SIZES = (300, 4096, 4097, 61440, 61441)


@dataclass
class FitCase:
    name: str
    pts: np.ndarray                 # (n, 2) x, y
    sizes: List[int]                # members per cluster, clusters in ascending order of their smallest index
    grid_ok: bool                   # a grid variant of the clustering accepts the instance (else: point-level fallback)
    seg_class: int                  # launch class of the segment in k_fit_gather: 0 above 16 384 points, 1 above 8 192, else 2
    R0: float = 3.0
    Rd: float = 0.001
    roots: Optional[np.ndarray] = None   # smallest index per cluster, ascending (where the builder plants it)

    @property
    def n(self):
        return len(self.pts)

    @property
    def n_clusters(self):
        return len(self.sizes)


# ---------------------------------------------------------------------------------------------------- pool helper
def pool_from_segments(segs, pad=3):
    """segs: list of (n_i,3) fp64 arrays -> pool tensors + base/cnt (with gaps)."""
    base, cnt, chunks, cur = [], [], [], 0
    for s in segs:
        base.append(cur)
        cnt.append(len(s))
        chunks.append(np.asarray(s, np.float64).reshape(-1, 3))
        chunks.append(np.full((pad, 3), 777.0))
        cur += len(s) + pad
    allp = np.concatenate(chunks) if chunks else np.zeros((0, 3))
    cap = max(len(allp), 1) + 8
    P = np.full((cap, 3), 555.0)
    P[:len(allp)] = allp
    return P, np.array(base, np.int64), np.array(cnt, np.int32), cap


# ---------------------------------------------------------------------------------------------------- pieces
def lshape(rng, cx, cy, L, Wd, yaw, n, sigma=0.02):
    """n noisy points on two sides of an L x Wd rectangle turned by yaw, in a random order."""
    k = n // 2
    e1 = np.stack([rng.uniform(-L / 2, L / 2, k), np.full(k, -Wd / 2)], 1)
    e2 = np.stack([np.full(n - k, -L / 2), rng.uniform(-Wd / 2, Wd / 2, n - k)], 1)
    q = np.vstack([e1, e2]) + rng.normal(0, sigma, (n, 2))
    R = np.array([[math.cos(yaw), -math.sin(yaw)], [math.sin(yaw), math.cos(yaw)]])
    return (q @ R.T + np.array([cx, cy]))[rng.permutation(n)]


def lattice(nx, ny, pitch, cx=0.0, cy=0.0):
    """nx x ny points `pitch` apart, centred on (cx, cy)."""
    gx = (np.arange(nx) - (nx - 1) / 2.0) * pitch + cx
    gy = (np.arange(ny) - (ny - 1) / 2.0) * pitch + cy
    xx, yy = np.meshgrid(gx, gy)
    return np.stack([xx.ravel(), yy.ravel()], 1)


def _seg_class(n):
    return 0 if n > 16384 else (1 if n > 8192 else 2)


def _mix(parts, order):
    """parts: one (m_k, 2) array per planted cluster; order: a permutation of all their points.  -> the points in that
    order, the clusters' sizes in ascending order of their smallest index (= the order of the rows), those indices."""
    pts = np.concatenate(parts)
    cid = np.concatenate([np.full(len(p), k) for k, p in enumerate(parts)])
    pts, cid = pts[order], cid[order]
    first = np.full(len(parts), len(pts))
    np.minimum.at(first, cid, np.arange(len(pts)))
    by_root = np.argsort(first)
    return pts, [len(parts[k]) for k in by_root], first[by_root]


# ---------------------------------------------------------------------------------------------------- (a)
def edge_size_cases():
    """One instance per member count in EDGE_SIZES: a noisy L shape, one cluster."""
    rng = np.random.default_rng(1401)
    out = []
    for i, m in enumerate(EDGE_SIZES):
        a = 2 * math.pi * i / len(EDGE_SIZES)
        pts = lshape(rng, 25.0 * math.cos(a), 25.0 * math.sin(a), 4.6 + 0.2 * i, 1.9 + 0.05 * i, 0.3 * i - 1.2, m)
        out.append(FitCase("edge%d" % m, pts, [m], True, _seg_class(m)))
    return out


TIE_SIZES = (64, 65, 2048, 2049, 4097)                  # k_fit_tiny | k_fit_medium, LDS | big list, a second staging chunk
TIE_HEADINGS = ((2.0, 44), (1.0, 89), (0.75, 119), (0.7, 128))   # (dtheta_deg, headings)
TIE_FOLD = 60
# (headings, case): (heading index of the oracle, of the library) where the two pick DIFFERENT members of the tied set --
# measured on the library as it was before the tie test existed and unchanged since.  The tied costs agree to the last
# bits and the library's three sweeps add up in another order than numpy's (lanes striding the points against pairwise
# sums), so either index is an arg-max of "the reference's formula"; which one numpy lands on is not reproducible on the
# GPU.  These combinations are left out of the GPU test (tests/test_gpu_fit_edges.py), the other fourteen are in it.
TIE_DISAGREE = {(44, "tie64"): (14, 29), (44, "tie4097"): (2, 5), (89, "tie64"): (28, 58),
                (119, "tie64"): (101, 77), (119, "tie2049"): (103, 63), (119, "tie4097"): (61, 5)}


def ring_tie_cases():
    """One instance per member count in TIE_SIZES, one cluster each: concentric regular 60-gons with a random phase per
    ring, radii in (0.4, 2.4] m, and the n mod 60 points left over exactly on the common centre.  The set is invariant
    under turns of 6 degrees, so at every heading count of TIE_HEADINGS several headings share the best cost up to the
    last bits: the search has to go through tier 2, the band rule and the reference's three-sweep cost."""
    out = []
    for n in TIE_SIZES:
        rng = np.random.default_rng(n)
        cx, cy = 10.0 + n % 7, -4.0
        k, extra = divmod(n, TIE_FOLD)
        parts = []
        for i in range(k):
            a = rng.uniform(0, 2 * np.pi) + 2 * np.pi * np.arange(TIE_FOLD) / TIE_FOLD
            r = 0.4 + 2.0 * (i + 1) / k
            parts.append(np.stack([cx + r * np.cos(a), cy + r * np.sin(a)], 1))
        parts.append(np.tile([[cx, cy]], (extra, 1)))
        out.append(FitCase("tie%d" % n, np.vstack(parts), [n], True, _seg_class(n)))
    return out


def ring_tie_cases_at(n_theta):
    """The ring cases the GPU test runs at this heading count: all but those of TIE_DISAGREE."""
    return [c for c in ring_tie_cases() if (n_theta, c.name) not in TIE_DISAGREE]


def tier1_band(pts, dtheta_deg, tau=1e-8):
    """The indices of the headings that the two-tier search of fit_stage.hip re-scores: a float64 restatement of its
    two-sweep cost (variance = q/n - (s/n)^2 of the edge distances of E1 / E2) and of the band `tau * largest mag` under
    the best cost."""
    dtheta = np.deg2rad(dtheta_deg)
    x, y = pts[:, 0], pts[:, 1]
    cost, mag = [], []
    for theta in np.arange(0.0, np.pi / 2.0 - dtheta, dtheta):
        ct, st = np.cos(theta), np.sin(theta)
        c1, c2 = x * ct + y * st, x * (-st) + y * ct
        d1 = np.minimum(np.abs(c1.max() - c1), np.abs(c1 - c1.min()))
        d2 = np.minimum(np.abs(c2.max() - c2), np.abs(c2 - c2.min()))
        v = m = 0.0
        for e in (d1[d1 < d2], d2[~(d1 < d2)]):
            if len(e):
                v -= np.mean(e * e) - np.mean(e) ** 2
                m += np.mean(e * e)
        cost.append(v)
        mag.append(m)
    cost = np.array(cost)
    return np.nonzero(cost >= cost.max() - tau * max(mag))[0]


# ---------------------------------------------------------------------------------------------------- (b)
def long_cases():
    """[0]: 16 385 points, one cluster.  [1]: one cluster of 16 384, one of 300 and twelve singletons, interleaved."""
    rng = np.random.default_rng(1402)
    one = FitCase("long16385", lshape(rng, -14.0, 9.0, 7.0, 2.5, 0.7, 16385), [16385], True, 0)
    parts = [lshape(rng, 10.0, 5.0, 6.5, 2.4, -0.4, 16384), lshape(rng, -25.0, 10.0, 4.4, 1.8, 1.1, 300)]
    parts += [p[None, :] for p in lattice(4, 3, 5.0, 37.5, -25.0)]
    n = sum(len(p) for p in parts)
    pts, sizes, roots = _mix(parts, rng.permutation(n))
    return [one, FitCase("long16384+300+12", pts, sizes, True, 0, roots=roots)]


# ---------------------------------------------------------------------------------------------------- (c)
GK = 512                            # clusters per pass of k_fit_gather


def many_cluster_case():
    """529 singletons on a 4 m lattice (R <= 3.07 there) and clusters of 2, 65, 300 and 2 049 members outside it: 533
    clusters, two passes of the gather.  The cluster of 65 has its smallest index among the first 512 roots, the other
    three have theirs beyond the 512th, and the members of every one of them are spread over the instance."""
    rng = np.random.default_rng(1403)
    single = lattice(23, 23, 4.0)
    single = single[rng.permutation(len(single))]
    c2 = np.array([[60.0, 0.0], [60.7, 0.7]])
    c65 = lshape(rng, -60.0, 0.0, 4.2, 1.8, 0.5, 65)
    c300 = lshape(rng, 0.0, 60.0, 4.6, 1.9, -0.3, 300)
    c2049 = lshape(rng, 0.0, -60.0, 6.0, 2.2, 1.0, 2049)
    parts = [p[None, :] for p in single] + [c2, c65, c300, c2049]
    off = np.cumsum([0] + [len(p) for p in parts])
    idx = lambda k: np.arange(off[k], off[k + 1])
    ns = len(single)
    head = np.concatenate([np.arange(520), idx(ns + 1)[:30]])                 # 520 singletons + 30 members of c65
    tail = np.setdiff1d(np.arange(off[-1]), head)
    order = np.concatenate([head[rng.permutation(len(head))], tail[rng.permutation(len(tail))]])
    pts, sizes, roots = _mix(parts, order)
    multi = [(m, k) for k, m in enumerate(sizes) if m > 1]                    # (members, rank of the root)
    assert sorted(m for m, _ in multi) == [2, 65, 300, 2049]
    assert sum(k < GK for _, k in multi) >= 1 and sum(k >= GK for _, k in multi) >= 2, multi
    assert GK < len(sizes) < 2 * GK
    return FitCase("many533", pts, sizes, True, 2, roots=roots)


def singleton_case(nx=33, ny=32):
    """nx * ny singletons on a 4 m lattice (more than 1 024: three passes of the gather), in a random order."""
    rng = np.random.default_rng(1404)
    pts = lattice(nx, ny, 4.0)
    pts = pts[rng.permutation(len(pts))]
    return FitCase("single%d" % len(pts), pts, [1] * len(pts), True, 2, roots=np.arange(len(pts)))


# ---------------------------------------------------------------------------------------------------- (d)
def fallback_case(n):
    """An instance no grid variant takes (wider than 12 288 cells): two dense strips, 2 m wide and up to 250 m long, and
    isolated points on a jittered 8 m lattice over +-300 m, interleaved.  n points; 4 096 / 61 440 are the last sizes of
    the fallback's first two forms.  (Strips, not blobs: few of the pairs are linked, which keeps the oracle's O(n^2)
    sweep at a few seconds for 61 441 points.)"""
    rng = np.random.default_rng(1500 + n)
    n_out = min(n // 3, 700)
    n_a = (n - n_out) // 2
    n_b = n - n_out - n_a
    half = min(125.0, n_a / 8.0)                                   # at least four points per metre of strip
    ys = (0.0, 40.0)

    def strip(yc, m):
        return np.stack([rng.uniform(-half, half, m), yc + rng.uniform(-1.0, 1.0, m)], 1)
    sites = lattice(75, 75, 8.0)
    far = np.ones(len(sites), bool)
    for yc in ys:
        far &= (np.abs(sites[:, 1] - yc) > 15.0) | (np.abs(sites[:, 0]) > half + 15.0)
    sites = sites[far]
    out = sites[rng.choice(len(sites), n_out, replace=False)] + rng.uniform(-1.0, 1.0, (n_out, 2))
    parts = [strip(ys[0], n_a), strip(ys[1], n_b)] + [p[None, :] for p in out]
    pts, sizes, roots = _mix(parts, rng.permutation(n))
    return FitCase("fallback%d" % n, pts, sizes, False, _seg_class(n), roots=roots)


def _linked(pi, pj, R0, Rd):
    """The reference's link rule, in its arithmetic: (d <= R_i or d <= R_j), and d <= R_i alone."""
    dx, dy = pi[0] - pj[0], pi[1] - pj[1]
    d = np.sqrt(dx * dx + dy * dy)
    Ri = R0 + Rd * np.sqrt(pi[0] * pi[0] + pi[1] * pi[1])
    Rj = R0 + Rd * np.sqrt(pj[0] * pj[0] + pj[1] * pj[1])
    return bool(d <= Ri or d <= Rj), bool(d <= Ri)


ASYM_STEPS = (-4, -2, -1, 0, 1, 2, 4)
ASYM_ANGLES = (0.0, 0.7, 2.3, -1.9)


def asym_link_cases(R0, Rd, r_i, grid_ok):
    """Two dense blobs on a ray from the origin whose ONLY possible link is the pair (p_i at range r_i, the end of the
    near blob; p_j, the start of the far one): |p_i p_j| is larger than R_i and within a few ulps of R_j = R0 + Rd |p_j|,
    so the two blobs are one cluster only through the farther point's radius.  One instance per ray angle and step:
    p_j sits ASYM_STEPS ulps of its range away from the last range at which the pair is still linked.  Every other pair
    across the gap is farther apart than both radii by 4 cm or more."""
    rng = np.random.default_rng(1600 + int(1000 * Rd))
    out = []
    for ai, ang in enumerate(ASYM_ANGLES):
        u = np.array([math.cos(ang), math.sin(ang)])
        w = np.array([-u[1], u[0]])
        pi = r_i * u
        lo, hi = r_i + R0, (R0 + r_i) / (1.0 - Rd) + 0.5          # linked at lo (d = R0 <= R_i), not linked at hi
        assert _linked(pi, lo * u, R0, Rd)[0] and not _linked(pi, hi * u, R0, Rd)[0]
        while np.nextafter(lo, np.inf) < hi:                       # the last range that is still linked
            mid = 0.5 * (lo + hi)
            if _linked(pi, mid * u, R0, Rd)[0]:
                lo = mid
            else:
                hi = mid
        for st in ASYM_STEPS:
            r_j = lo
            for _ in range(abs(st)):
                r_j = np.nextafter(r_j, np.inf if st > 0 else -np.inf)
            pj = r_j * u
            both, by_i = _linked(pi, pj, R0, Rd)
            assert not by_i                                        # never through the nearer point's radius
            m = 300
            A = np.outer(rng.uniform(r_i - 4.0, r_i - 0.05, m), u) + np.outer(rng.uniform(-1.5, 1.5, m), w)
            B = np.outer(rng.uniform(r_j + 0.05, r_j + 4.0, m), u) + np.outer(rng.uniform(-1.5, 1.5, m), w)
            A[0], B[0] = pi, pj
            parts = [np.concatenate([A, B])] if both else [A, B]
            pts, sizes, roots = _mix(parts, rng.permutation(2 * m))
            out.append(FitCase("asym_a%d_%+d" % (ai, st), pts, sizes, grid_ok, 2, R0, Rd, roots=roots))
    assert {len(c.sizes) for c in out} == {1, 2}                   # both outcomes occur
    return out


def asym_far_cases():
    """Rd = 0.05, ranges about 28.5 and 33.16 m: R_i = 4.425 < d = 4.658 ~ R_j; R_max is above 4.238 there, so no grid
    variant is eligible and the point-level fallback decides."""
    return asym_link_cases(3.0, 0.05, 28.5, False)


def asym_near_cases():
    """The twin at Rd = 0.001 around the origin (ranges 1 and 4.004 m: R_i = 3.001 < d = 3.004 ~ R_j): grid path."""
    return asym_link_cases(3.0, 0.001, 1.0, True)


# ---------------------------------------------------------------------------------------------------- expected rows
def expected_rows(segs, M, classes, iscar, boxes, scores, ocalibs, oparams):
    """The 24-column engine rows of dfu3d_lshape_fit from the oracle, ordered by (view, instance, cluster): columns 0-15
    from generate_anns; score, members, heading, extents (c1min, c2min, c1max, c2max) and root from the clusters and the
    rectangle generate_anns itself worked with (recorded on the way, so that the search runs once per cluster).
    -> (rows, labels): labels[s][i] = smallest index of the cluster of point i of segment s, from the same clusters."""
    from oracle import penet_oracle as O
    seg_fn, rect_fn = O.range_segmentation, O.rectangle_search
    rec = {}

    def seg_rec(*a, **k):
        rec["clusters"] = seg_fn(*a, **k)
        rec["rects"] = []
        return rec["clusters"]

    def rect_rec(*a, **k):
        r = rect_fn(*a, **k)
        rec["rects"].append(r)
        return r
    out, labels = [], []
    O.range_segmentation, O.rectangle_search = seg_rec, rect_rec
    try:
        for s, pts in enumerate(segs):
            rec["clusters"] = []
            name = "Car" if iscar[s] else "Truck"
            for r in O.generate_anns(name, pts, classes[s], np.asarray(boxes[s], np.float32), ocalibs[s // M], oparams,
                                     inst=s % M):
                ids = rec["clusters"][r.cluster]
                th, _, _, cc = rec["rects"][r.cluster]
                out.append(np.concatenate([[s // M, s % M, r.cluster, r.cls], r.as_vector(),
                                           [float(np.float32(scores[s])), len(ids), th, cc[0], cc[1], cc[2], cc[3],
                                            ids[0]]]))
            lab = np.full(len(pts), -1, np.int32)
            for ids in rec["clusters"]:
                lab[ids] = ids[0]
            labels.append(lab)
    finally:
        O.range_segmentation, O.rectangle_search = seg_fn, rect_fn
    return np.array(out, np.float64).reshape(-1, ROW_COLS), labels


def sort_rows(R):
    return R[np.lexsort((R[:, 2], R[:, 1], R[:, 0]))]


def assert_row_matches(got, exp, dtheta):
    """One row of the library against its expected row, all 24 columns: integers, member count, root and the heading
    INDEX equal; box numbers (4-15) and extents (19-22) within 1e-9; the score is the instance's float32."""
    key = tuple(int(v) for v in exp[:3])
    assert [int(v) for v in got[:4]] == [int(v) for v in exp[:4]] and np.array_equal(got[:4], np.round(got[:4])), key
    np.testing.assert_allclose(got[4:16], exp[4:16], rtol=1e-9, atol=1e-9, err_msg=str(key))
    assert got[16] == exp[16], (key, got[16], exp[16])
    assert (got[17], got[23]) == (exp[17], exp[23]), (key, got[17], got[23], exp[17], exp[23])
    assert int(round(got[18] / dtheta)) == int(round(exp[18] / dtheta)), (key, got[18], exp[18])
    np.testing.assert_allclose(got[19:23], exp[19:23], rtol=1e-9, atol=1e-9, err_msg=str(key))


def assert_rows_match(got, exp, dtheta):
    """got: the library's rows in any order; exp: expected_rows().  Same count, every row compared."""
    assert got.shape == exp.shape, (got.shape, exp.shape)
    for g, e in zip(sort_rows(got), exp):
        assert_row_matches(g, e, dtheta)
