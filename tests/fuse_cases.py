"""Inputs of the ball-query fuse and statistical-filter edge tests (tests/test_gpu_fuse_stat_edges.py,
tests/test_fuse_cases_host.py): instances planted where k_ball_flags, k_seg_compact, k_knn_mean and k_stat_flags of
segment_stage.hip take another path -- pairs right at the threshold, neighbours only across a cell border, every phase
of the quantised pruning bound, chains of hundreds of nodes, hash slots shared by several cells, LiDAR counts on the
edges of the two table builds and of the brute-force tiles, LiDAR points beyond the quantised range (the fallback),
non-finite coordinates, lists the radius filter empties, and segment sizes around the k-NN tiles.
Every builder is seeded and returns plain numpy.  The kernel's cell arithmetic is restated below (quant, cell_of,
in_range, candidate_cells, prune_sum, bh_hash, table_slots) so that tests/test_fuse_cases_host.py can prove on the CPU
that a case is what it claims to be; expected results come from the oracle, none are stored."""
from dataclasses import dataclass, field
from typing import List

import numpy as np

# ---------------------------------------------------------------------------------------------------- the kernel's numbers
OFF = 65536.0                        # quantised coordinates are stored with this offset
Q_LO, Q_HI = 64.0, 131000.0          # a LiDAR point is in range iff Q_LO <= f < Q_HI on every axis
Q_MAX = 131071.0                     # 17 bits
CELL_SHIFT = 5                       # a cell is 32 units wide
SMALL_MAX, BIG_MAX = 1024, 4096      # LiDAR points the table of the small / the big build holds
SMALL_BT, BIG_BT = 256, 1024         # queries per workgroup tile
SMALL_TILE, BIG_TILE = SMALL_MAX // 3, BIG_MAX // 3      # LiDAR points per brute-force tile: 341, 1365
COMPACT_STEP = 2048                  # positions per step of k_seg_compact
PRUNE_BOUND = 257
KNN_QT, KNN_PT, KNN_MAX = 128, 1024, 64                  # k_knn_mean: queries per workgroup, points per LDS tile, largest k


def unit(C):
    """u = C (1 + 1e-5) / 16: sixteen units per C."""
    return C * (1.0 + 1e-5) / 16.0


def quant(x, C):
    """floor(x / u) + 65536 as the kernel forms it: the product with inv = 16 / (C (1 + 1e-5)).  float64, not clamped."""
    inv = 16.0 / (C * (1.0 + 1e-5))
    return np.floor(np.asarray(x, np.float64) * inv) + OFF


def in_range(pts, C):
    """(n,) bool: the point's three quantised coordinates lie in [64, 131000) (NaN / Inf: False)."""
    f = quant(pts, C)
    with np.errstate(invalid="ignore"):
        return ((f >= Q_LO) & (f < Q_HI)).all(-1)


def cell_of(pts, C):
    """(n, 3) int64 cell coordinates (quantised coordinate >> 5) of in-range points."""
    return quant(pts, C).astype(np.int64) >> CELL_SHIFT


def candidate_cells(q, C):
    """The cells the kernel walks for query q: per axis the cells of floor((q -+ C') / u) + 65536, C' = C (1 + 1e-6),
    clamped to the 17 bits.  -> list of (cx, cy, cz)."""
    Cq = C * (1.0 + 1e-6)
    lo = np.clip(quant(np.asarray(q) - Cq, C), 0.0, Q_MAX).astype(np.int64) >> CELL_SHIFT
    hi = np.clip(quant(np.asarray(q) + Cq, C), 0.0, Q_MAX).astype(np.int64) >> CELL_SHIFT
    return [(x, y, z) for x in range(lo[0], hi[0] + 1) for y in range(lo[1], hi[1] + 1) for z in range(lo[2], hi[2] + 1)]


def prune_sum(a, q, C):
    """The quantised lower bound of the node test: sum over the axes of max(|qa - qq| - 1, 0)^2; a node is tested exactly
    iff this is <= 257."""
    d = np.abs(quant(a, C) - quant(q, C))
    e = np.maximum(d - 1.0, 0.0)
    return (e * e).sum(-1)


def _umul24(a, b):
    return ((int(a) & 0xFFFFFF) * (int(b) & 0xFFFFFF)) & 0xFFFFFFFF


def bh_hash(cx, cy, cz):
    h = _umul24(cx, 0x9E3779) ^ _umul24(cy, 0x85EBCB) ^ _umul24(cz, 0xC2B2AF)
    h ^= h >> 15
    h ^= h >> 7
    return h


def table_slots(na):
    slots = 256
    while slots < 2 * na:
        slots <<= 1
    return slots


def slot_of_cells(cells, na):
    """(m,) slot of every cell (m, 3) in the table of an instance with na LiDAR points."""
    mask = table_slots(na) - 1
    return np.array([bh_hash(*c) & mask for c in cells], np.int64)


def dist(q, A):
    """(len(A),) distances as the oracle forms them: sqrt((dx*dx + dy*dy) + dz*dz)."""
    d = np.asarray(q, np.float64)[None, :] - np.asarray(A, np.float64).reshape(-1, 3)
    s = d[:, 0] * d[:, 0]
    s = s + d[:, 1] * d[:, 1]
    s = s + d[:, 2] * d[:, 2]
    return np.sqrt(s)


# ---------------------------------------------------------------------------------------------------- cases
@dataclass
class FuseCase:
    """One dfu3d_ballquery_fuse call: instance s has the LiDAR list A[s] and the pseudo list B[s]."""
    name: str
    C: float
    A: List[np.ndarray]
    B: List[np.ndarray]
    expect: str = "mix"              # "mix": at least 20 kept and 20 dropped queries; "all" / "none": every query kept / dropped
    fallback: List[bool] = field(default_factory=list)       # per instance: a LiDAR point lies outside the quantised range
    info: dict = field(default_factory=dict)                  # what the builder planted, for the host test

    def __post_init__(self):
        self.A = [np.ascontiguousarray(a, np.float64).reshape(-1, 3) for a in self.A]
        self.B = [np.ascontiguousarray(b, np.float64).reshape(-1, 3) for b in self.B]
        if not self.fallback:
            self.fallback = [False] * len(self.A)


def _unit_vec(rng):
    v = rng.normal(0, 1, 3)
    return v / np.linalg.norm(v)


def _lattice_sites(rng, n, pitch, centre, jitter=0.1):
    """n distinct sites of a cubic lattice of the given pitch around `centre`, each moved by up to jitter * pitch per axis,
    in a random order: two sites are at least (1 - 2 jitter) pitch apart."""
    m = 1
    while m ** 3 < n:
        m += 1
    g = (np.arange(m) - (m - 1) / 2.0) * pitch
    xx, yy, zz = np.meshgrid(g, g, g, indexing="ij")
    sites = np.stack([xx.ravel(), yy.ravel(), zz.ravel()], 1)[rng.permutation(m ** 3)[:n]]
    return sites + rng.uniform(-jitter, jitter, (n, 3)) * pitch + np.asarray(centre, np.float64)


# ------------------------------------------------------------------ isolated threshold pairs
THRESHOLD_RELS = (1e-5, 1e-7, 1e-9, 1e-12, 1e-15, 3e-16, 0.0)
THRESHOLD_CS = (0.05, 0.1, 0.5)
_S2, _S3 = 1.0 / np.sqrt(2.0), 1.0 / np.sqrt(3.0)
DIRECTIONS = (("x", (1, 0, 0)), ("y", (0, 1, 0)), ("z", (0, 0, 1)), ("xy", (_S2, _S2, 0)), ("xz", (_S2, 0, -_S2)),
              ("yz", (0, -_S2, _S2)), ("xyz", (_S3, _S3, _S3)), ("random", None))
# pair centres in metres at C = 0.1 (scaled with C: the quantised range is +-4092 C)
THRESHOLD_CENTRES = ((0.0, 0.0, 0.0), (40.0, 40.0, 40.0), (-40.0, -40.0, -40.0), (400.0, 400.0, 400.0),
                     (-400.0, -400.0, -400.0), (400.0, -400.0, 40.0))


def threshold_case(C):
    """One LiDAR point and one query per pair, at distance C (1 +- rel); one instance per centre (all in the table path),
    and the pairs around the origin once more behind a LiDAR point beyond the range (the brute-force predicate)."""
    rng = np.random.default_rng(4100 + int(round(C * 1000)))
    scale = C / 0.1
    pitch = max(1.0, 8.0 * C)
    A, B = [], []
    for centre in THRESHOLD_CENTRES:
        specs = [(d, rel, sign) for _, d in DIRECTIONS for rel in THRESHOLD_RELS for sign in (-1.0, 1.0)]
        a = _lattice_sites(rng, len(specs), pitch, np.array(centre) * scale)
        q = np.empty_like(a)
        for k, (d, rel, sign) in enumerate(specs):
            u = _unit_vec(rng) if d is None else np.array(d, np.float64)
            if rng.random() < 0.5:
                u = -u
            q[k] = a[k] + u * (C * (1.0 + sign * rel))
        A.append(a[rng.permutation(len(a))])
        B.append(q[rng.permutation(len(q))])
    far = np.array([[5000.0 * scale, 0.0, 0.0]])
    A.append(np.concatenate([A[0][:50], far, A[0][50:]]))
    B.append(B[0].copy())
    return FuseCase("threshold_C%g" % C, C, A, B, fallback=[False] * len(THRESHOLD_CENTRES) + [True], info=dict(pitch=pitch))


# ------------------------------------------------------------------ phase sweep of the pruning bound
PHASE_DIRS = (("x", (1.0, 0.0, 0.0)), ("xy", (_S2, _S2, 0.0)), ("xyz", (_S3, _S3, _S3)))


def phase_case(C):
    """Pairs at distance C (1 - 1e-9) along an axis, a face diagonal and the body diagonal; the LiDAR point of a pair sits
    at phase (k + 1/2) / 64 of a unit, k = 0 .. 63, on the x, the y, the z axis alone and on all three at once, so that
    the quantised differences take every value the bound can see.  Every query must be kept."""
    rng = np.random.default_rng(4200 + int(round(C * 1000)))
    u = unit(C)
    pitch = max(1.0, 8.0 * C)
    specs = [(d, axes, k) for _, d in PHASE_DIRS for axes in ((0,), (1,), (2,), (0, 1, 2)) for k in range(64)]
    sites = _lattice_sites(rng, len(specs), pitch, (3.0 * pitch, -5.0 * pitch, 2.0 * pitch), jitter=0.0)
    a = np.empty_like(sites)
    q = np.empty_like(sites)
    for i, (d, axes, k) in enumerate(specs):
        ph = rng.uniform(0.05, 0.95, 3)                   # the phase of the axes that are not swept
        for ax in axes:
            ph[ax] = (k + 0.5) / 64.0
        a[i] = (np.round(sites[i] / u) + ph) * u
        q[i] = a[i] + np.array(d) * (C * (1.0 - 1e-9))
    p = rng.permutation(len(a))
    return FuseCase("phase_C%g" % C, C, [a[p]], [q[rng.permutation(len(q))]], expect="all", info=dict(pitch=pitch))


# ------------------------------------------------------------------ neighbours only across cell borders
def border_configs():
    """(delta per axis): the neighbour's cell minus the query's cell; one, two or three axes, low and high side."""
    out = []
    for dx in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dz in (-1, 0, 1):
                if (dx, dy, dz) != (0, 0, 0):
                    out.append((dx, dy, dz))
    return out


BORDER_KINDS = ("near", "reach", "far")


def border_case(C=0.1):
    """Per configuration and place three queries whose nearest LiDAR point lies in the adjacent cell: "near" -- query and
    neighbour on either side of the border, 0.5 C apart (kept); "reach" -- the query 0.93 C from the border on one of the
    axes and the neighbour just behind it, 0.95 C apart: the far end of the query's quantised range (kept); "far" -- 1.05 C
    apart (dropped).  For a kept query that neighbour is the only LiDAR point within C.  All eight cells a query's walk
    visits hold a LiDAR point farther than C.  info["queries"]: (index in B, neighbour's index in A, delta, kind)."""
    rng = np.random.default_rng(4300)
    u = unit(C)
    places = ((0, 0, 0), (-300, 170, -45), (1950, -1950, 1900), (-2000, -2020, -1980))     # cell offsets from the origin's cell
    A, B, queries = [], [], []
    site = 0
    for place in places:
        for ci, delta in enumerate(border_configs()):
            for kind in BORDER_KINDS:
                cell0 = np.array(place) + 2048 + 12 * np.array([site % 5, (site // 5) % 5, site // 25]) - 24
                site = (site + 1) % 125
                axes = [ax for ax, d in enumerate(delta) if d]
                long_ax = axes[ci % len(axes)]                     # "reach": the axis on which the query stands back
                step = (1.05 if kind == "far" else 0.5) * C / np.sqrt(len(axes))
                qp, ap = np.empty(3), np.empty(3)
                for ax, d in enumerate(delta):
                    lo = (cell0[ax] * 32 - OFF) * u                # low border of the query's cell
                    back, over = 0.02 * C, step - 0.02 * C         # the query's distance from the border, the neighbour's
                    if kind == "reach":
                        back, over = (0.93 * C, 0.01 * C) if ax == long_ax else (0.02 * C, 0.1 * C)
                    if d > 0:
                        qp[ax] = lo + 32 * u - back
                        ap[ax] = lo + 32 * u + over
                    elif d < 0:
                        qp[ax] = lo + back
                        ap[ax] = lo - over
                    else:
                        qp[ax] = lo + (8.0 if rng.random() < 0.5 else 24.0) * u      # a quarter in: the walk takes a second cell
                        ap[ax] = qp[ax] + 0.01 * C
                queries.append((len(B), len(A), delta, kind))
                A.append(ap)
                B.append(qp)
                for cell in candidate_cells(qp, C):                # a LiDAR point farther than C in every cell of the walk
                    lo = (np.array(cell) * 32 - OFF) * u
                    for _ in range(1000):
                        p = lo + rng.uniform(0.02, 0.98, 3) * 32 * u
                        if dist(qp, p)[0] > 1.2 * C:
                            A.append(p)
                            break
                    else:
                        raise AssertionError("no place for a distractor")
    A, B = np.array(A), np.array(B)
    pa, pb = rng.permutation(len(A)), rng.permutation(len(B))
    ia, ib = np.argsort(pa), np.argsort(pb)
    queries = [(int(ib[qi]), int(ia[ai]), delta, kind) for qi, ai, delta, kind in queries]
    return FuseCase("borders", C, [A[pa]], [B[pb]], info=dict(queries=queries))


# ------------------------------------------------------------------ dense cells and shared slots
def dense_case(C=0.1):
    """260 LiDAR points in the middle of ONE cell (a chain of hundreds of nodes), LiDAR point 0 in the low corner of that
    cell and the last one in its high corner.  Queries outside the cell see only point 0 (the end of the chain), only the
    last point (its head), or nothing; queries inside see the crowd.  info: cell, and per kind the query indices."""
    rng = np.random.default_rng(4400)
    u = unit(C)
    W = 32 * u
    cell = np.array([2048 + 7, 2048 - 3, 2048 + 1])
    lo = (cell * 32 - OFF) * u
    crowd = lo + rng.uniform(0.3, 0.7, (260, 3)) * W
    first, last = lo + 0.02 * W, lo + 0.98 * W
    A = np.concatenate([first[None], crowd, last[None]])
    def octant(n, r0, r1, sign):
        v = np.abs(rng.normal(0, 1, (n, 3)))
        v /= np.linalg.norm(v, axis=1)[:, None]
        return sign * v * rng.uniform(r0, r1, (n, 1)) * C
    tail = first + octant(30, 0.3, 0.9, -1.0)
    head = last + octant(30, 0.3, 0.9, 1.0)
    none = np.concatenate([first + octant(25, 1.1, 1.5, -1.0), last + octant(25, 1.1, 1.5, 1.0)])
    inside = lo + rng.uniform(0.35, 0.65, (30, 3)) * W
    B = np.concatenate([tail, head, none, inside])
    kind = np.array(["tail"] * 30 + ["head"] * 30 + ["none"] * 50 + ["inside"] * 30)
    p = rng.permutation(len(B))
    return FuseCase("dense", C, [A], [B[p]], info=dict(cell=tuple(int(c) for c in cell), kind=kind[p]))


def shared_slot_case(C=0.1):
    """1024 LiDAR points, nearly every one in a cell of its own, over 2048 slots: several occupied cells share a slot."""
    rng = np.random.default_rng(4500)
    a = rng.uniform(-30.0, 30.0, (1024, 3))
    near = a[rng.integers(0, 1024, 400)] + rng.normal(0, 0.6 * C, (400, 3))
    B = np.concatenate([near, rng.uniform(-30.0, 30.0, (200, 3))])
    return FuseCase("shared_slots", C, [a], [B[rng.permutation(len(B))]])


# ------------------------------------------------------------------ class and tile boundaries
def _planted_lists(rng, na, pattern, centre, C):
    """na LiDAR points on a jittered lattice of pitch 5 C (any two at least 4 C apart) and one query per entry of `pattern`:
    True = 0.5 C from a LiDAR point (kept), False = 1.6 C from one (dropped: at least 2.4 C from every other)."""
    a = _lattice_sites(rng, na, 5.0 * C, centre)
    pattern = np.asarray(pattern, bool)
    tg = rng.integers(0, na, len(pattern))
    v = rng.normal(0, 1, (len(pattern), 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    b = a[tg] + v * np.where(pattern, 0.5 * C, 1.6 * C)[:, None]
    return a, b


def alternating(nb):
    """Runs of three kept / three dropped queries, the phase flipped at every 2048-position step of k_seg_compact."""
    i = np.arange(nb)
    return ((i // 3) % 2 == 0) ^ ((i // COMPACT_STEP) % 2 == 1)


BOUNDARY_INSTANCES = (    # (LiDAR count, pseudo count, pattern)
    (1, 255, "mix"), (2, 256, "mix"), (255, 257, "mix"), (256, 255, "all"), (257, 256, "none"), (1023, 257, "mix"),
    (1024, 2047, "alt"),                                                              # the small build
    (1025, 1023, "mix"), (4095, 1024, "all"), (4096, 1025, "none"), (1025, 2049, "alt"), (4096, 2048, "alt"),     # the big build
    (4097, 1023, "mix"), (4097, 1024, "all"), (4097, 1025, "none"), (4097, 2049, "alt"), (4200, 4097, "alt"))    # brute force


def boundary_case(C=0.1):
    rng = np.random.default_rng(4600)
    A, B, patterns = [], [], []
    for k, (na, nb, pat) in enumerate(BOUNDARY_INSTANCES):
        pattern = {"mix": rng.random(nb) < 0.5, "all": np.ones(nb, bool), "none": np.zeros(nb, bool), "alt": alternating(nb)}[pat]
        a, b = _planted_lists(rng, na, pattern, rng.uniform(-40, 40, 3), C)
        A.append(a)
        B.append(b)
        patterns.append(pattern)
    return FuseCase("boundaries", C, A, B, info=dict(patterns=patterns))


# ------------------------------------------------------------------ fallback to brute force
FALLBACK_COUNTS = (1, 341, 342, 683, 1024, 1366, 2731, 4096)    # LiDAR counts: tiles of 341 (small build) and 1365 (big build)
FALLBACK_FAR_AT = ("first", "last", "first", "middle", "middle", "first", "first", "middle")    # never alone in the last tile


def fallback_case(C=0.1):
    """Ordinary instances with ONE LiDAR point at 500 m (beyond the range), first, in the middle or last in the list.  The
    first 40 queries of every instance have their neighbour in the LAST brute-force tile only (info["last_tile"]: the list
    positions of its ordinary points); the last query sits next to the far point.  Then an instance all of whose points
    are near 500 m, and an in-range one whose LiDAR points lie just inside the range on either side, with queries beyond
    it."""
    rng = np.random.default_rng(4700)
    scale = C / 0.1
    A, B, fb, last_tile = [], [], [], []
    for na, far_where in zip(FALLBACK_COUNTS, FALLBACK_FAR_AT):
        tile = SMALL_TILE if na <= SMALL_MAX else BIG_TILE
        far_at = {"first": 0, "middle": (na - 1) // 2, "last": na - 1}[far_where]
        t0 = ((na - 1) // tile) * tile                                   # list position at which the last tile starts
        nb = 300
        pattern = rng.random(nb) < 0.5
        pattern[:40] = True
        far = np.array([500.0 * scale, -3.0, 2.0])
        if na == 1:
            a = far[None]
            b = rng.uniform(-5, 5, (nb, 3)) * scale
            lt_pos = np.zeros(0, np.int64)
        else:
            pos = np.array([i for i in range(na) if i != far_at])        # list positions of the ordinary points
            lt = np.nonzero(pos >= t0)[0]                                # the ordinary points of the last tile
            a, b = _planted_lists(rng, na - 1, pattern, rng.uniform(-30, 30, 3), C)
            tg = lt[rng.integers(0, len(lt), 40)]
            v = rng.normal(0, 1, (40, 3))
            v /= np.linalg.norm(v, axis=1)[:, None]
            b[:40] = a[tg] + v * 0.5 * C
            a = np.concatenate([a[:far_at], far[None], a[far_at:]])
            lt_pos = pos[lt]
        b[-1] = far + np.array([0.3, -0.2, 0.1]) * C                     # a query beyond the range, next to the far point
        A.append(a)
        B.append(b)
        fb.append(True)
        last_tile.append(lt_pos)
    # every point near 500 m, LiDAR and queries alike
    pattern = rng.random(300) < 0.5
    a, b = _planted_lists(rng, 300, pattern, np.array([500.0, 500.0, 500.0]) * scale, C)
    A.append(a); B.append(b); fb.append(True); last_tile.append(np.zeros(0, np.int64))
    # LiDAR points just inside the range on the high and on the low side, queries beyond it; the table path
    u = unit(C)
    hi_edge, lo_edge = (Q_HI - OFF) * u, (Q_LO - OFF) * u
    a, b = [], []
    for k in range(120):
        ax, side = k % 3, (k // 3) % 2
        p = rng.uniform(-100, 100, 3) * scale
        p[ax] = hi_edge - rng.uniform(0.05, 0.4) * C if side else lo_edge + rng.uniform(0.05, 0.4) * C
        step = np.zeros(3)
        step[ax] = (1.0 if side else -1.0) * (0.6 if k % 2 else 1.3) * C
        a.append(p)
        b.append(p + step)                                              # beyond the range: 0.6 C (kept) or 1.3 C (dropped) away
    for k in range(30):                                                  # and far beyond all 17 bits
        p = rng.uniform(-100, 100, 3) * scale
        p[k % 3] = (1.0 if k % 2 else -1.0) * rng.uniform(450.0, 5000.0) * scale
        b.append(p)
    A.append(np.array(a)); B.append(np.array(b)); fb.append(False); last_tile.append(np.zeros(0, np.int64))
    return FuseCase("fallback", C, A, B, fallback=fb, info=dict(last_tile=last_tile))


# ------------------------------------------------------------------ non-finite values
def nonfinite_case(C=0.1):
    """Queries with a NaN, +Inf or -Inf coordinate (dropped) among ordinary ones, in the small table, the big table and
    brute force; then the same three sizes with a NaN and / or an Inf LiDAR point, which forces the fallback."""
    rng = np.random.default_rng(4800)
    A, B, fb, bad_q = [], [], [], []
    for k, (na, bad_a) in enumerate(((300, ()), (2000, ()), (4200, ()), (300, (np.nan,)), (2000, (np.inf,)), (4200, (np.nan, -np.inf)))):
        pattern = rng.random(200) < 0.5
        a, b = _planted_lists(rng, na, pattern, rng.uniform(-20, 20, 3), C)
        bad = np.zeros(len(b), bool)
        for j, val in enumerate((np.nan, np.inf, -np.inf) * 3):
            i = 7 + 11 * j
            b[i, j % 3] = val
            bad[i] = True
        b[150] = np.nan
        b[151] = np.inf
        bad[150:152] = True
        for j, val in enumerate(bad_a):
            a[(37 + 1000 * j) % na, (k + j) % 3] = val
        A.append(a); B.append(b); fb.append(len(bad_a) > 0); bad_q.append(bad)
    return FuseCase("nonfinite", C, A, B, fallback=fb, info=dict(bad_q=bad_q))


def plain_cases():
    """Every case that goes through the plain dfu3d_ballquery_fuse."""
    cases = [threshold_case(C) for C in THRESHOLD_CS] + [phase_case(C) for C in THRESHOLD_CS]
    cases += [border_case(), dense_case(), shared_slot_case(), boundary_case(), fallback_case(), nonfinite_case()]
    return cases


# ------------------------------------------------------------------ joint mode: radius filter over both lists, then the fuse
@dataclass
class JointCase:
    name: str
    A: List[np.ndarray]
    B: List[np.ndarray]
    ra: np.ndarray
    rb: np.ndarray
    info: dict = field(default_factory=dict)


def joint_case():
    """Four instances (radius filter with nb_points = 1, then the joint fuse at C = 0.1):
    0  a LiDAR pair at 600 m, 0.3 m apart: the filter keeps it, so the fallback runs with the LiDAR mask;
    1  4200 LiDAR points, the first 1400 isolated: the whole first brute-force tile (1365) is dropped, later ones are kept;
    2  4200 LiDAR points, all isolated: the fuse is skipped, every filtered pseudo point stays;
    3  1024 LiDAR points, all isolated: the table is built with nothing in it, the fuse is skipped."""
    rng = np.random.default_rng(4900)
    A, B = [], []
    # 0
    a = np.concatenate([rng.normal(0, 2.0, (500, 3)), np.array([[600.0, 1.0, -2.0], [600.3, 1.0, -2.0]])])
    a = a[rng.permutation(len(a))]
    pair = np.nonzero(a[:, 0] > 500.0)[0]
    b = rng.normal(0, 2.0, (800, 3))
    b[:400] = a[rng.integers(0, len(a), 400)] + rng.normal(0, 0.06, (400, 3))
    b[400:420] = a[pair[0]] + rng.normal(0, 0.06, (20, 3))
    A.append(a); B.append(b[rng.permutation(len(b))])
    # 1
    iso = _lattice_sites(rng, 1400, 8.0, (0.0, 0.0, 300.0))
    body = rng.normal(0, 1.0, (2800, 3))
    a = np.concatenate([iso, body])
    b = rng.normal(0, 1.0, (1500, 3))
    b[:700] = body[rng.integers(0, len(body), 700)] + rng.normal(0, 0.06, (700, 3))
    b[700:760] = iso[rng.integers(0, len(iso), 60)] + rng.normal(0, 0.03, (60, 3))     # isolated too: the filter drops them
    A.append(a); B.append(b[rng.permutation(len(b))])
    # 2, 3
    for n in (4200, 1024):
        a = _lattice_sites(rng, n, 8.0, (0.0, 0.0, 0.0))
        b = rng.normal(0, 30.0, (1200, 3))
        b[:300] = a[rng.integers(0, n, 300)] + rng.normal(0, 0.06, (300, 3))
        A.append(a); B.append(b[rng.permutation(len(b))])
    ra = np.array([3.0, 3.0, 3.0, 3.0])
    rb = np.array([0.6, 3.0, 3.0, 0.6])
    return JointCase("joint", A, B, ra, rb, info=dict(pair=pair, first_tile=BIG_TILE, n_isolated=1400))


# ---------------------------------------------------------------------------------------------------- statistical filter
STAT_SIZES = (0, 1, 2, 3, 20, 127, 128, 129, 1023, 1024, 1025, 2100)
STAT_KS = (1, 2, 5, 30, 63, 64)
STAT_RATIOS = (-1.0, 0.0, 0.3, 2.0, 1e9)


def clustered_points(rng, n, spread=0.5, outliers=0.1):
    k = max(1, n // 40)
    centers = rng.uniform(-20, 20, (k, 3)) * np.array([1, 1, 0.1])
    p = centers[rng.integers(0, k, n)] + rng.normal(0, spread, (n, 3))
    m = rng.random(n) < outliers
    p[m] = rng.uniform(-80, 80, (int(m.sum()), 3))
    return p


def stat_segments():
    """-> (segments, enable): every size of STAT_SIZES enabled, each followed by a disabled segment of 50 points."""
    rng = np.random.default_rng(5100)
    segs, enable = [], []
    for n in STAT_SIZES:
        segs.append(clustered_points(rng, n))
        enable.append(1)
        segs.append(clustered_points(rng, 50))
        enable.append(0)
    return segs, np.array(enable, np.int32)


def duplicate_segments():
    """-> (segments, enable): 40 copies of one point; 300 clustered points with 35 copies of one point among them (at
    info positions); a disabled segment of duplicates."""
    rng = np.random.default_rng(5200)
    same = np.repeat(rng.normal(0, 1, (1, 3)), 40, 0)
    mixed = clustered_points(rng, 300)
    where = np.sort(rng.permutation(300)[:35])
    mixed[where] = mixed[where[0]]
    off = np.repeat(rng.normal(0, 1, (1, 3)), 45, 0)
    return [same, mixed, off], np.array([1, 1, 0], np.int32), where
