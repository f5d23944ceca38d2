"""Inputs shared by the f-3 tests (tests/test_gpu_iou3d.py, tests/test_gpu_iou3d_edges.py, tests/test_oracle_iou3d.py,
tests/test_rect_overlap_vertex_bound.py): the random scenes of the NMS cases and the families of box pairs on which
polygon clippers go wrong.  No expected values live here."""
import numpy as np

f32 = np.float32
PI = f32(np.pi)


def random_boxes(rng, n, spread=20.0):
    b = np.zeros((n, 7), f32)
    b[:, :2] = rng.uniform(-spread, spread, (n, 2))
    b[:, 2] = rng.uniform(-2, 0, n)
    b[:, 3:6] = rng.uniform(0.6, 6.0, (n, 3))
    b[:, 6] = rng.uniform(-6.5, 6.5, n)
    return b


# ---- NMS scenes ------------------------------------------------------------------------------------------------------
# (n, nominal threshold, pre_maxsize, normal).  The threshold a case runs at is the midpoint of the widest gap between
# oracle IoU values within +-0.01 of the nominal one (oracle.widest_gap_threshold), so that no pair is ambiguous.
NMS_CASES = [(1, 0.1, None, False), (63, 0.1, None, False), (64, 0.01, None, False), (65, 0.3, None, False),
             (700, 0.1, None, False), (4096, 0.2, 3000, False), (2500, 0.7, None, False), (900, 0.25, None, True),
             # more than 4096 boxes: slots 1..7 of k_nms_reduce's running set
             (4097, 0.2, None, False), (8192, 0.2, None, False), (12345, 0.3, None, False), (32768, 0.2, None, False),
             (8192, 0.25, None, True),
             # pre_maxsize beyond n, and one that cuts just past a 4096 boundary
             (500, 0.2, 1000, False), (6000, 0.2, 4097, False)]
LARGE_NMS = {4097, 8192, 12345, 32768, 6000}    # about 4 m^2 of ground per box: a third to a half is suppressed
DENSE_2500 = (2500, 0.7, 2.0)                   # (n, nominal threshold, spread): 2500 boxes on 4 m x 4 m


def nms_scene(n, spread=None):
    """Boxes and distinct scores of the case with n boxes (seeded by n).  No seed had to be skipped: the half-width of
    the threshold gap exceeds 1e-5 for every case at its first seed (asserted on the oracle in the tests)."""
    rng = np.random.default_rng(100 + n)
    if spread is None:
        spread = np.sqrt(n) if n in LARGE_NMS else 4.0 * np.sqrt(n) ** 0.5 + 4.0
    boxes = random_boxes(rng, n, spread)
    scores = rng.permutation(n).astype(f32) / n             # distinct -> the order is unambiguous
    return boxes, scores


# ---- degenerate pairs ------------------------------------------------------------------------------------------------
def _ulps(x, k):
    x = f32(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, f32(np.inf) if k > 0 else f32(-np.inf))
    return x


def _base(rng, spread=6.0):
    return random_boxes(rng, 1, spread)[0]


def _shift(b, du, dv):
    """b moved by du along its first axis and dv along its second one (float32 result)."""
    o = b.copy()
    c, s = np.cos(np.float64(b[6])), np.sin(np.float64(b[6]))
    o[0] = f32(b[0] + du * c - dv * s)
    o[1] = f32(b[1] + du * s + dv * c)
    return o


def _fam_identical(rng, g):
    return [g] * 8, [g] * 8


def _fam_quarter_turns(rng, g):
    B = []
    for turn in [f32(k) * PI / f32(2) for k in range(-4, 5)] + [f32(2) * PI, -f32(2) * PI]:
        o = g.copy()
        o[6] = g[6] + turn                                       # float32: the turn is a multiple of pi / 2 up to an ulp
        B.append(o)
    return [g] * 4, B


def _fam_ulp(rng, g):
    def nudge():
        o = g.copy()
        for col in rng.choice([0, 1, 3, 4, 6], size=rng.integers(1, 4), replace=False):
            o[col] = _ulps(o[col], rng.choice([-4, -3, -2, -1, 1, 2, 3, 4]))
        return o
    return [g] + [nudge() for _ in range(7)], [g] + [nudge() for _ in range(7)]


def _zero_variants(rng, g):
    out = []
    for cols in ((3,), (4,), (3, 4)):
        for place in (0, 1, 2):
            o = g.copy()
            o[list(cols)] = 0
            if place == 1:                                    # the line / point lies on an edge of g
                o = _shift(o, g[3] / 2 if 3 in cols else 0.0, g[4] / 2 if 4 in cols else 0.0)
            elif place == 2:                                  # somewhere inside, turned
                o = _shift(o, rng.uniform(-0.4, 0.4) * g[3], rng.uniform(-0.4, 0.4) * g[4])
                o[6] = f32(rng.uniform(-3.2, 3.2))
            out.append(o)
    return out


def _fam_zero_b(rng, g):
    return [g] * 4, _zero_variants(rng, g)


def _fam_zero_a(rng, g):
    return _zero_variants(rng, g), [g] * 4


def _fam_zero_both(rng, g):
    z = _zero_variants(rng, g)
    return z, z[::-1]


def _fam_shared_edge(rng, g):
    B = []
    for du, dv in ((1, 0), (-1, 0), (0, 1), (0, -1),             # a full edge
                   (1, 0.5), (-1, -0.5), (0.5, 1), (-0.5, -1),  # half an edge
                   (1, 1), (-1, 1), (1, -1), (-1, -1)):         # one corner
        B.append(_shift(g, du * np.float64(g[3]), dv * np.float64(g[4])))
    return [g] * 4, B


def _fam_inside(rng, g):
    B = []
    for _ in range(8):
        o = g.copy()
        k = rng.uniform(0.2, 0.45)                               # half diagonal of o < shortest half extent of g
        o[3:5] = f32(k * min(g[3], g[4]))
        o = _shift(o, rng.uniform(-0.1, 0.1) * g[3], rng.uniform(-0.1, 0.1) * g[4])
        o[6] = f32(rng.uniform(-6.5, 6.5))
        B.append(o)
    return [g] * 4, B


def _fam_cross(rng, g):
    a = g.copy(); a[3], a[4] = 6.0, 0.5
    sq = g.copy(); sq[3], sq[4] = 1.0, 1.0
    B, A = [], [a, a, a, a, sq, sq]
    for turn in (PI / f32(2), -PI / f32(2), PI / f32(4), f32(3) * PI / f32(4)):
        o = a.copy(); o[6] = a[6] + turn
        B.append(o)
    for turn in (PI / f32(4), -PI / f32(4)):                      # unit squares: an octagon of area 8 (sqrt 2 - 1) / 4
        o = sq.copy(); o[6] = sq[6] + turn
        B.append(o)
    return A, B


def _fam_sliver(rng, g):
    a = g.copy(); a[3], a[4] = 6.0, 6.0
    B = []
    for _ in range(8):
        o = a.copy(); o[3], o[4] = 9.0, 1e-3
        o = _shift(o, rng.uniform(-2, 2), rng.uniform(-2, 2))
        o[6] = f32(rng.choice([a[6], a[6] + PI / f32(2), rng.uniform(-3.2, 3.2)]))
        B.append(o)
    return [a] * 4, B


def _fam_unequal(rng, g):
    a = g.copy(); a[3], a[4] = 60.0, 60.0
    B = []
    for place in range(8):
        o = g.copy(); o[3], o[4] = 0.05, 0.05
        o[6] = f32(rng.uniform(-3.2, 3.2))
        if place >= 4:                                           # on the big box's edge / corner
            o = _shift(a, 30.0, (place - 5) * 30.0 if place < 7 else rng.uniform(-30, 30))
            o[3], o[4] = 0.05, 0.05
        B.append(o)
    return [a] * 4, B


FAMILIES = dict(identical=_fam_identical, quarter_turns=_fam_quarter_turns, ulp=_fam_ulp, zero_b=_fam_zero_b,
                zero_a=_fam_zero_a, zero_both=_fam_zero_both, shared_edge=_fam_shared_edge, inside=_fam_inside,
                cross=_fam_cross, sliver=_fam_sliver, unequal=_fam_unequal)


def family_blocks(rng, groups=4, names=None):
    """-> (A (N,7), B (M,7), blocks): blocks[name] is a list of (row indices, column indices); every row of such a block
    paired with every column of it is a pair of that family (built from one base box).  Rows and columns of different
    blocks are ordinary unrelated pairs."""
    A, B, blocks = [], [], {}
    for name in (names or FAMILIES):
        blocks[name] = []
        for _ in range(groups):
            a, b = FAMILIES[name](rng, _base(rng))
            blocks[name].append((np.arange(len(A), len(A) + len(a)), np.arange(len(B), len(B) + len(b))))
            A += list(a); B += list(b)
    return np.asarray(A, f32).reshape(-1, 7), np.asarray(B, f32).reshape(-1, 7), blocks


def family_pairs(rng, groups, names=None):
    """The pairs of `family_blocks` one by one -> (a (p,7), b (p,7), family index (p,), names)."""
    A, B, blocks = family_blocks(rng, groups, names)
    ia, ib, fam = [], [], []
    for k, name in enumerate(blocks):
        for rows, cols in blocks[name]:
            r, c = np.meshgrid(rows, cols, indexing="ij")
            ia.append(r.ravel()); ib.append(c.ravel()); fam.append(np.full(r.size, k))
    ia, ib = np.concatenate(ia), np.concatenate(ib)
    return A[ia], B[ib], np.concatenate(fam), list(blocks)


def to_fmt5(b7):
    """(n,7) -> (n,5) [cx cy w h angle] of rotate_iou.py describing the same footprints (its angle turns clockwise)."""
    b7 = np.asarray(b7, f32)
    return np.stack([b7[:, 0], b7[:, 1], b7[:, 3], b7[:, 4], -b7[:, 6]], 1).astype(f32)


def rigid_motion(b, shift, turn):
    """Boxes turned about the origin by `turn` and then moved by `shift` (float64 arithmetic, float32 result)."""
    o = np.asarray(b, np.float64).copy()
    c, s = np.cos(turn), np.sin(turn)
    o[:, 0] = b[:, 0] * c - b[:, 1] * s + shift[0]
    o[:, 1] = b[:, 0] * s + b[:, 1] * c + shift[1]
    o[:, 6] = b[:, 6] + turn
    return o.astype(f32)
