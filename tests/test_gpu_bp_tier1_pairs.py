"""GPU tests of tier 1 of k_bp_bin on pixel PAIRS: a thread's four consecutive pixels of a row are classified as two
register pairs with packed float32 arithmetic, their table cells are gathered together, and the decisions are formed with
selects.  Nothing of that may change a result: every case compares the voxels of a whole pass (n_vox, vox_pix, bits, xyz)
bit for bit with oracle/penet_oracle.py and runs the pass twice (the helpers of test_gpu_bp_empty_tiles.py, 70 x 132
views: 3 x 3 tiles, the last tile column 4 pixels wide, the last tile row 6 rows high).

The share of pixels tier 1 leaves undecided is a condition of its own: each one costs the middle tier's instructions on
one wave while three wait.  PARENT_UNDECIDED holds undecided / tried of stages.selftest_classify measured on the parent
of this change (commit 6b75791, one MI355X, the very calls of test_selftest_share_and_no_wrong_decision); the change must
stay within 1.5 x of each."""
import numpy as np
import pytest

from oracle import penet_oracle as O
from tests.test_gpu_bp_empty_tiles import (H, W, _assert_oracle, _bp_oracle, _bp_run, _oracle_calib, below,  # noqa: F401
                                           st)

pytestmark = pytest.mark.gpu

PPT = 4                                   # pixels per thread and row of k_bp_bin: two pairs (0, 1) and (2, 3)
VS = float(np.float32(0.002))             # bin width in theta and phi, RMIN the first edge (stages.make_geom's defaults)
RMIN = -5.0
# a dead partner: no depth, negative, NaN, below depth_min = 0.001 -- and +inf, which passes the depth test and must
# come out as "no voxel" without touching its neighbour
DEAD = [0.0, -1.0, float("nan"), float("inf"), 0.0005]


def _live(depth):
    return np.where(depth >= 0.5, depth, np.float32(7.5)).astype(np.float32)


def _lone_maps(depth):
    """Views 0, 1: in every piece of four pixels ONE is live, the other three are DEAD values; views 2, 3: ONE is a DEAD
    value, the other three live.  -> maps, [(view, position in the piece, index into DEAD)] of every piece."""
    out = _live(depth)
    combos = []
    rows, groups = np.meshgrid(np.arange(H), np.arange(W // PPT), indexing="ij")
    for v in range(4):
        pos = (groups + rows + v) % PPT
        kind = (groups + 2 * rows + v) % len(DEAD)
        for k in range(PPT):
            odd = (pos == k) if v >= 2 else (pos != k)             # the pixels that get the dead value
            vals = np.array(DEAD, np.float32)[kind]
            out[v, :, k::PPT] = np.where(odd, vals, out[v, :, k::PPT])
        combos += [(v, int(p), int(q)) for p, q in zip(pos.ravel(), kind.ravel())]
    return out, combos


def test_lone_maps_cover_every_position_and_dead_value():
    """(no GPU work) every position of the four x every dead value, both as the only live pixel of its piece (views
    0, 1) and as the only dead one (views 2, 3)."""
    _, combos = _lone_maps(np.full((4, H, W), 5.0, np.float32))
    for views in ((0, 1), (2, 3)):
        assert {(p, q) for v, p, q in combos if v in views} == {(p, q) for p in range(PPT) for q in range(len(DEAD))}


@pytest.mark.parametrize("key_axis", [1, 2])
def test_dead_partner_neither_poisons_nor_drops_its_neighbour(st, below, key_axis):
    depth, cal, masks = below
    maps, _ = _lone_maps(depth)
    want = [_bp_oracle(maps[v], cal[v], masks[v], key_axis) for v in range(4)]
    assert all(len(w[0]) > 300 for w in want)
    _assert_oracle(_bp_run(st, maps, cal, masks, key_axis), want)


def _angles(depth_v, cal):
    """fp64 theta, phi and x of every pixel of a map without a zero, as the reference computes them -> (H, W) each."""
    rows, cols, pl = O.backproject(np.array(depth_v), _oracle_calib(cal), 0.0)
    assert len(rows) == depth_v.size
    _, theta, phi = O.to_sphere_coords(pl)
    return theta.reshape(depth_v.shape), phi.reshape(depth_v.shape), pl[:, 0].reshape(depth_v.shape)


def _on_edges(depth_v, cal, axis):
    """Every pixel's depth moved so that its fp64 theta (axis 0) or phi (axis 1) lands on the nearest bin edge, pair
    partners on opposite sides of theirs (even columns 5e-10 rad above, odd columns below): Newton steps on a float64
    map, then the best of the float32 depths around the solution.  -> float32 map, |angle - edge| of every pixel."""
    side = np.where(np.arange(W) % 2 == 0, 1.0, -1.0)[None, :]
    d = _live(depth_v).astype(np.float64)
    a0 = _angles(d, cal)[axis]
    target = RMIN + np.round((a0 - RMIN) / VS) * VS + side * 5e-10
    for _ in range(8):
        a = _angles(d, cal)[axis]
        slope = (_angles(d * (1.0 + 1e-6), cal)[axis] - a) / (d * 1e-6)
        with np.errstate(all="ignore"):
            step = np.where(np.abs(slope) > 1e-9, (a - target) / slope, 0.0)
        d = np.clip(d - step, 0.3, 150.0)
    best = d.astype(np.float32)
    dist = np.abs(_angles(best, cal)[axis] - target)
    for ulps in (-2, -1, 1, 2):
        cand = (best.view(np.int32) + ulps).view(np.float32)
        dc = np.abs(_angles(cand, cal)[axis] - target)
        best, dist = np.where(dc < dist, cand, best), np.minimum(dc, dist)
    return best, np.abs(_angles(best, cal)[axis] - (target - side * 5e-10))


@pytest.fixture(scope="module")
def hard(below):
    """Four views of depths chosen against tier 1's margins -> depth, calibrations, masks, the edge distances."""
    depth, cal, masks = below
    maps = np.empty_like(depth)
    k = np.arange(W)[None, :] + np.arange(H)[:, None]
    maps[0] = np.where(k % 2 == 0, 0.6, 60.0)                         # 100 x apart inside every pair
    maps[1] = np.where(k % PPT == 0, 0.6, 60.0)                       # one near pixel among three far ones, every position
    maps[2], dist_t = _on_edges(depth[2], cal[2], 0)
    maps[3], dist_p = _on_edges(depth[3], cal[3], 1)
    return maps.astype(np.float32), cal, masks, dist_t, dist_p


def test_edge_maps_reach_the_edges(hard):
    """(no GPU work) float32 depths cannot put every pixel within 1e-9 rad of an edge (one ulp of the depth moves the
    angle by 1e-8 .. 1e-7 rad): enough of them get there, and all of them are closer than any margin tier 1 uses at
    these depths (1.5e-6 and up)."""
    _, _, _, dist_t, dist_p = hard
    for dist in (dist_t, dist_p):
        assert (dist < 1e-9).sum() >= 50, (dist < 1e-9).sum()
        assert np.median(dist) < 2e-7


@pytest.mark.parametrize("key_axis", [1, 2])
def test_depths_100x_apart_and_pixels_on_bin_edges(st, hard, key_axis):
    maps, cal, masks, _, _ = hard
    want = [_bp_oracle(maps[v], cal[v], masks[v], key_axis) for v in range(4)]
    assert all(len(w[0]) > 300 for w in want)
    _assert_oracle(_bp_run(st, maps, cal, masks, key_axis), want)


def _sideways_view():
    """A camera that looks along +y: x = d w + e crosses zero inside the depth range for the columns around the
    principal point.  Every such pixel gets the float32 depth nearest to the crossing, its pair partner one 3 ulp off."""
    from dfu3d_amd import synth
    cal = synth.make_calibration(90.0, H, W, np.random.default_rng(7))
    one, two = np.full((H, W), 1.0), np.full((H, W), 2.0)
    x1, x2 = _angles(one, cal)[2], _angles(two, cal)[2]
    with np.errstate(all="ignore"):
        root = 1.0 - x1 / (x2 - x1)                                   # x is linear in d
    hit = (root > 0.6) & (root < 90.0)
    d = np.where(hit, root, 7.5).astype(np.float32)
    off = np.where(np.arange(W) % 2 == 0, 0, 3)[None, :] * np.where(np.arange(H) % 2 == 0, 1, -1)[:, None]
    d = (d.view(np.int32) + off.astype(np.int32)).view(np.float32)
    return d, cal, hit


def _centred_view(below):
    """View 0 with the principal point ON a pixel: column 66 has u == cu, row 35 has v == cv, exactly."""
    from dfu3d_amd import synth
    depth, cal, _ = below
    P2 = np.array(cal[0].P2, np.float32)
    P2[0, 2], P2[1, 2] = 66.0, 35.0
    c = synth.Calibration({"P2": P2, "R0": cal[0].R0, "Tr_velo2cam": cal[0].V2C})
    assert float(c.cu) == 66.0 and float(c.cv) == 35.0
    return _live(depth[0]), c


@pytest.mark.parametrize("key_axis", [1, 2])
def test_x_near_zero_and_zero_numerators_of_the_key(st, below, key_axis):
    _, _, masks = below
    d0, c0, hit = _sideways_view()
    assert hit.sum() >= 100
    x = _angles(d0, c0)[2]
    assert (np.abs(x[hit]) < 1e-5).all() and (x[hit] > 0).any() and (x[hit] < 0).any()
    d1, c1 = _centred_view(below)
    maps, cal = np.stack([d0, d1]), [c0, c1]
    want = [_bp_oracle(maps[v], cal[v], masks[v], key_axis) for v in range(2)]
    assert len(want[1][0]) > 300
    pix = want[1][0]
    assert (pix % W == 66).any() and (pix // W == 35).any()            # voxels whose key has a zero numerator
    _assert_oracle(_bp_run(st, maps, cal, masks[:2], key_axis), want)


# undecided / tried of stages.selftest_classify on the parent commit 6b75791 (2 000 000 pixels, seed 9, camera yaw 0 at
# 900 x 1600, key_axis 1): [geometry][depth range]
RANGES = [(0.5, 5.0), (5.0, 120.0), (0.5, 120.0)]
NARROW = dict(theta_min=1.2, z_max=0.5, vsize=(200.0, 0.0005, 0.0005), vgrid=(1, 20000, 20000))    # bins 4 x narrower
PARENT_UNDECIDED = {"bench": [14499 / 2e6, 178912 / 2e6, 172787 / 2e6], "narrow": [145173 / 2e6, 278848 / 2e6, 274057 / 2e6]}


@pytest.mark.parametrize("name,kw", [("bench", {}), ("narrow", NARROW)])
def test_selftest_share_and_no_wrong_decision(st, name, kw):
    from dfu3d_amd import synth
    cal = synth.make_calibration(0.0, 900, 1600, np.random.default_rng(3))
    geom, _ = st.make_geom(**kw)
    for (d_lo, d_hi), parent in zip(RANGES, PARENT_UNDECIDED[name]):
        r = st.selftest_classify(cal.record(), 900, 1600, geom, 1, 2_000_000, seed=9, d_lo=d_lo, d_hi=d_hi)
        share = r["undecided"] / r["tried"]
        print("selftest_classify %s d in [%g, %g): %r undecided share %.6f (parent %r)" % (name, d_lo, d_hi, r, share, parent))
        assert r["tried"] == 2_000_000 and r["wrong"] == 0, (name, d_lo, d_hi, r)
        assert share <= 1.5 * parent, (name, d_lo, d_hi, share, parent)
