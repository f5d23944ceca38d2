"""The packed node test of k_ball_flags (segment_stage.hip) restated in numpy, for tests/test_ball_packed_bound_host.py and
tests/test_gpu_ball_packed_nodes.py.  A node's word holds the LiDAR point's position inside its cell, one byte per axis:
(i & 31) + 160.  The query's word for cell u holds Q' = q - 32 u + 32 per axis.  One 32-bit subtraction, an xor with
0x00808080 and a signed 4 x 8-bit dot product of the word with itself give dx^2 + dy^2 + dz^2 of the quantised
differences; a node goes to the exact fp64 predicate iff that sum is <= D2_MAX.  tests/fuse_cases.py restates the cell
arithmetic (quant, candidate_cells, ...) and the parent filter's bound (PRUNE_BOUND = 257 on sum max(|d| - 1, 0)^2)."""
import numpy as np

from tests import fuse_cases as F

D2_MAX = 314                         # the packed filter: sum d^2 <= 314
NODE_BIAS = 160                      # node byte = (i & 31) + 160
END_BYTES = 0x00FFFFFF               # the end node every chain runs into: bytes that fail against every Q'
R_LO, R_HI = -17, 48                 # q - 32 u of a packed query, every cell u of its walk
QB_LO, QB_HI = R_LO + 32, R_HI + 32  # Q' in [15, 80]


def node_bytes(i):
    """(n, 3) quantised coordinates (integers) -> (n,) uint32 node words."""
    i = np.asarray(i, np.int64)
    b = (i & 31) + NODE_BIAS
    return (b[..., 0] | (b[..., 1] << 8) | (b[..., 2] << 16)).astype(np.uint32)


def query_bytes(q, cell):
    """Quantised query (.., 3) and cell coordinates (.., 3) -> uint32 query words; the bytes must lie in [15, 80]."""
    r = np.asarray(q, np.int64) - 32 * np.asarray(cell, np.int64) + 32
    assert ((r >= QB_LO) & (r <= QB_HI)).all()
    return (r[..., 0] | (r[..., 1] << 8) | (r[..., 2] << 16)).astype(np.uint32)


def packed_d2(nb, qb):
    """The kernel's three instructions on uint32 words: subtract, xor, signed dot product of the four bytes with themselves."""
    u = (np.asarray(nb, np.uint32) - np.asarray(qb, np.uint32)) ^ np.uint32(0x00808080)
    s = np.zeros(u.shape, np.int64)
    for k in range(4):
        byte = ((u >> np.uint32(8 * k)) & np.uint32(0xFF)).astype(np.int64)
        byte = np.where(byte >= 128, byte - 256, byte)
        s += byte * byte
    return s


def walk_of(x, C):
    """One coordinate of queries (n,) -> (q, x0, x1, qin): the quantised position and the first / last cell of the walk on
    that axis, as the kernel forms them (clamped to the 17 bits); rows whose range misses the 17 bits get x0 > x1."""
    x = np.asarray(x, np.float64)
    Cq = C * (1.0 + 1e-6)
    lo, hi, fq = F.quant(x - Cq, C), F.quant(x + Cq, C), F.quant(x, C)
    with np.errstate(invalid="ignore"):
        hit = (hi >= 0.0) & (lo <= F.Q_MAX)
        qin = (fq >= 0.0) & (fq <= F.Q_MAX)
    x0 = np.where(hit, np.clip(np.nan_to_num(lo), 0.0, F.Q_MAX), 32.0).astype(np.int64) >> F.CELL_SHIFT
    x1 = np.where(hit, np.clip(np.nan_to_num(hi), 0.0, F.Q_MAX), 0.0).astype(np.int64) >> F.CELL_SHIFT
    q = np.where(qin, np.nan_to_num(fq), 0.0).astype(np.int64)
    return q, x0, x1, qin & hit


def old_prune_sum(d):
    """The parent filter on integer quantised differences (.., 3): sum max(|d| - 1, 0)^2."""
    e = np.maximum(np.abs(np.asarray(d, np.int64)) - 1, 0)
    return (e * e).sum(-1)


def keep_by_oracle_distance(A, B, C):
    """(len(B),) bool: some LiDAR point lies at oracle distance < C (NaN compares false)."""
    if len(A) == 0:
        return np.ones(len(B), bool)
    with np.errstate(invalid="ignore"):
        return np.array([bool((F.dist(q, A) < C).any()) for q in B], bool)
