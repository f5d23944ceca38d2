"""The packed node test of k_ball_flags never rejects what the parent's filter accepted, its byte arithmetic never borrows
between bytes, and every pair within C passes it (CPU; the test is restated in tests/ball_packed.py)."""
import numpy as np
import pytest

from tests import ball_packed as P
from tests import fuse_cases as F


def test_every_difference_the_parent_filter_accepts_has_d2_at_most_314():
    """Exhaustive over d in [-63, 63]^3: sum max(|d| - 1, 0)^2 <= 257 implies sum d^2 <= 314, and 314 is reached."""
    g = np.arange(-63, 64)
    d = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    old = P.old_prune_sum(d) <= F.PRUNE_BOUND
    d2 = (d * d).sum(-1)
    new = d2 <= P.D2_MAX
    assert int(old.sum()) == 22503 and int(new.sum()) == 23439
    assert not (old & ~new).any()
    assert int(d2[old].max()) == P.D2_MAX
    # the parent capped every term at 31 before squaring: the same set (one capped term alone is 961)
    e = np.minimum(np.maximum(np.abs(d) - 1, 0), 31)
    assert np.array_equal((e * e).sum(-1) <= F.PRUNE_BOUND, old)


def test_bytes_never_borrow_and_the_xor_is_the_signed_difference():
    """Every node byte in [160, 191] (and the end node's 255) against every Q' in [15, 80]: the difference stays in
    [0, 255], its xor with 0x80 read as int8 is the quantised difference, and a whole word gives the three differences
    byte by byte with the fourth byte 0."""
    nb = np.concatenate([np.arange(160, 192), [255]])[:, None]
    qb = np.arange(P.QB_LO, P.QB_HI + 1)[None, :]
    diff = nb - qb
    assert diff.min() >= 0 and diff.max() <= 255
    s8 = (diff ^ 0x80).astype(np.uint8).view(np.int8).astype(np.int64)
    assert np.array_equal(s8, nb - 128 - qb)                  # = (i & 31) - (q - 32 u) for a node of cell u
    assert ((nb[-1] - 128 - qb) ** 2).min() > P.D2_MAX        # the end node fails on one byte alone
    # whole words: all three axes at once, every combination of the extreme and some middle values
    nv = np.array([160, 161, 175, 190, 191])
    qv = np.array([P.QB_LO, P.QB_LO + 1, 47, 48, P.QB_HI - 1, P.QB_HI])
    n3 = np.stack(np.meshgrid(nv, nv, nv, indexing="ij"), -1).reshape(-1, 3)
    q3 = np.stack(np.meshgrid(qv, qv, qv, indexing="ij"), -1).reshape(-1, 3)
    nw = (n3[:, 0] | (n3[:, 1] << 8) | (n3[:, 2] << 16)).astype(np.uint32)[:, None]
    qw = (q3[:, 0] | (q3[:, 1] << 8) | (q3[:, 2] << 16)).astype(np.uint32)[None, :]
    exp = (((n3[:, None, :] - 128) - q3[None, :, :]) ** 2).sum(-1)
    assert np.array_equal(P.packed_d2(nw, qw), exp)
    assert (P.packed_d2(np.uint32(P.END_BYTES), qw) > P.D2_MAX).all()


@pytest.mark.parametrize("C", F.THRESHOLD_CS)
def test_the_walk_rule_keeps_every_query_byte_in_range(C):
    """Queries over the whole quantised range, around every kind of cell border and at the clamped ends of the 17 bits:
    a query inside the 17 bits walks at most two cells per axis and q - 32 u lies in [-17, 48] for both, so Q' is a byte
    in [15, 80]; the kernel sends whatever fails this to the exact walk, which is then only the queries outside the 17 bits."""
    rng = np.random.default_rng(6100 + int(C * 1000))
    u = F.unit(C)
    cells = np.concatenate([rng.integers(0, 4096, 3000), [0, 1, 2, 4093, 4094, 4095] * 50])
    local = np.concatenate([rng.uniform(0, 32, 1500), rng.integers(0, 32, 1800) + rng.choice([1e-9, 0.5, 1 - 1e-9], 1800)])
    x = (cells * 32.0 + local - F.OFF) * u
    ends = np.concatenate([np.linspace(-40, 40, 4001), np.linspace(F.Q_MAX - 40, F.Q_MAX + 40, 4001)])
    x = np.concatenate([x, (ends - F.OFF) * u])
    q, x0, x1, qin = P.walk_of(x, C)
    assert qin.sum() > 6000 and (~qin).sum() > 1000
    assert (x1[qin] - x0[qin] <= 1).all() and (x1[qin] >= x0[qin]).all()
    r_lo, r_hi = q[qin] - 32 * x1[qin], q[qin] - 32 * x0[qin]
    assert r_lo.min() >= P.R_LO and r_hi.max() <= P.R_HI
    assert r_lo.min() <= -15 and r_hi.max() >= 46                       # the ends are met, within the slack for rounding
    # the clamped ends: the first and the last cell of the range were walked
    assert (x0[qin] == 0).any() and (x1[qin] == 4095).any()


@pytest.mark.parametrize("C", F.THRESHOLD_CS)
def test_every_pair_within_C_passes_the_packed_test(C):
    """Points around cell borders at the centres of fuse_cases.THRESHOLD_CENTRES, queries at 0.2 C .. C (1 - 1e-12) from
    them in random directions: the point's cell is in the query's walk and its packed sum is <= 314."""
    rng = np.random.default_rng(6200 + int(C * 1000))
    u = F.unit(C)
    worst = 0
    for centre in F.THRESHOLD_CENTRES:
        c = np.array(centre) * (C / 0.1)
        n = 4000
        cell = np.floor(c / (32 * u))[None, :] + rng.integers(-2, 3, (n, 3))
        local = np.where(rng.random((n, 3)) < 0.7, rng.choice([0.0, 31.0], (n, 3)) + rng.uniform(0, 1, (n, 3)), rng.uniform(0, 32, (n, 3)))
        a = (cell * 32.0 + local) * u
        v = rng.normal(0, 1, (n, 3))
        v /= np.linalg.norm(v, axis=1)[:, None]
        rel = rng.choice([0.2, 0.7, 0.97, 1 - 1e-5, 1 - 1e-9, 1 - 1e-12], n)
        b = a + v * (C * rel)[:, None]
        near = np.array([F.dist(b[k], a[k])[0] < C for k in range(n)])
        assert near.sum() > 0.9 * n
        ia, ca = F.quant(a, C).astype(np.int64), F.cell_of(a, C)
        walks = [P.walk_of(b[:, ax], C) for ax in range(3)]
        q = np.stack([w[0] for w in walks], 1)
        for ax, (_, x0, x1, qin) in enumerate(walks):
            assert qin.all()
            assert ((ca[:, ax] >= x0) & (ca[:, ax] <= x1))[near].all()       # the point's cell is walked
        d2 = P.packed_d2(P.node_bytes(ia[near]), P.query_bytes(q[near], ca[near]))
        assert np.array_equal(d2, ((ia[near] - q[near]) ** 2).sum(-1))       # the bytes give the quantised differences
        assert d2.max() <= P.D2_MAX
        worst = max(worst, int(d2.max()))
    assert worst >= 280                                                      # pairs near the bound were there
