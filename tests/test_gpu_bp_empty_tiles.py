"""GPU tests of the early exit of k_bp_bin: a workgroup (a tile of 64 x 32 pixels) whose pixels all fail the depth test
returns behind the set-up's barrier.  It may not lose a pixel: every case compares the voxels of the whole pass (n_vox,
vox_pix, bits, xyz) bit for bit with oracle/penet_oracle.py and runs the pass twice to show that the table was left
clean.  A tile whose live pixels tier 1 has all dropped has NO exit of its own (measured, not kept): its case checks
the path that falls through the window, the lists and the flush with nothing to do.

The views are 70 x 132 pixels: 3 x 3 tiles, the last tile column 4 pixels wide, the last tile row 6 rows high, cut
from a generated 180 x 320 scene with the principal point moved along."""
import numpy as np
import pytest
import torch

from oracle import penet_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
H, W = 70, 132
TW, TH = 64, 32                       # a workgroup's tile
BELOW, ACROSS = 96, 60                # first scene row of the window: all of it below the horizon / the horizon inside it
C0 = 160


@pytest.fixture(scope="module")
def st():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dfu3d_amd import stages
    return stages


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV).contiguous()


def _oracle_calib(c):
    return O.Calibration({"P2": c.P2, "R0": c.R0, "Tr_velo2cam": c.V2C})


def _bp_run(st, depth, cal, masks, key_axis=1, cap_vox=1 << 16, geom_kw=None):
    """One pass with every phase, twice (the second proves the table was left clean) -> n_vox, vox_pix, bits, xyz, status."""
    V, h, w = depth.shape
    geom, E = st.make_geom(**(geom_kw or {}))
    table = torch.empty(V * E * st.TABLE_ENTRY_BYTES, dtype=torch.uint8, device=DEV)
    st.bin_table_init(table, V * E)
    pw, bw = st.backproject_scratch_words(V, h, w, cap_vox, geom.max_points_per_voxel, geom)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)
    n_vox, vox_pix, bits = i32(V), i32(V * cap_vox), i32(V * cap_vox)
    x, y, z = f64(V * cap_vox), f64(V * cap_vox), f64(V * cap_vox)
    status = i32(1)
    M = masks.shape[1]
    calib = _t(np.stack([c.record() for c in cal]))
    n_inst = _t(np.full(V, M, np.int32))
    pix_bin, blk = i32(pw), i32(bw)
    out = []
    for rep in range(2):
        st.backproject_bin(_t(depth), calib, _t(masks), n_inst, V, M, h, w, geom, E, key_axis,
                           table, pix_bin, blk, cap_vox, n_vox, vox_pix, bits, x, y, z, status)
        torch.cuda.synchronize()
        out.append((n_vox.cpu().numpy().copy(), vox_pix.cpu().numpy().reshape(V, cap_vox).copy(),
                    bits.cpu().numpy().reshape(V, cap_vox).copy(),
                    torch.stack([x, y, z], 1).cpu().numpy().reshape(V, cap_vox, 3).copy(),
                    int(status.item())))
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    return out[0]


def _bp_oracle(depth_v, cal, masks_v, key_axis=1, params_kw=None):
    p = O.Params(**(params_kw or {}))
    rows, cols, pl = O.backproject(depth_v.copy(), _oracle_calib(cal), p.depth_min)
    zk = pl[:, 2] < p.z_max
    p0, r0, c0 = pl[zk], rows[zk], cols[zk]
    rep = O.voxel_sample(p0, p0[:, key_axis], p)
    pix = r0[rep] * depth_v.shape[1] + c0[rep]
    bits = np.zeros(len(rep), np.int64)
    for j in range(masks_v.shape[0]):
        bits |= (masks_v[j][r0[rep], c0[rep]] > 0).astype(np.int64) << j
    return pix, p0[rep], bits


def _assert_oracle(got, expected):
    n_vox, vox_pix, bits, xyz, status = got
    assert status == 0
    for v, (pix, pts, ob) in enumerate(expected):
        assert n_vox[v] == len(pix), (v, n_vox[v], len(pix))
        assert np.array_equal(vox_pix[v, :len(pix)], pix), v
        assert np.array_equal(bits[v, :len(pix)], ob), v
        assert np.array_equal(xyz[v, :len(pix)], pts), v


def _window(r0):
    """Four views of H x W pixels: rows r0 .., columns C0 .. of a generated 180 x 320 scene -> depth, calibrations, masks."""
    from dfu3d_amd import synth
    s = synth.make_scene(41, H=180, W=320, M=4, cams=4, dense=True, k_min=10, k_max=14)
    depth = np.ascontiguousarray(s.depth.numpy()[:, r0:r0 + H, C0:C0 + W])
    masks = np.ascontiguousarray(s.masks.numpy()[:, :, r0:r0 + H, C0:C0 + W])
    cal = []
    for c in s.calibs:
        P2 = np.array(c.P2, np.float32)
        P2[0, 2] -= C0
        P2[1, 2] -= r0
        cal.append(synth.Calibration({"P2": P2, "R0": c.R0, "Tr_velo2cam": c.V2C}))
    return depth, cal, masks


@pytest.fixture(scope="module")
def below():
    return _window(BELOW)


@pytest.fixture(scope="module")
def across():
    return _window(ACROSS)


# tile-local (row, col) of the single live pixel.  A thread holds two rows 16 apart (its "thread rows" 0 and 1), and wave w
# holds the tile rows with row % 4 == w (k_bp_bin: trow = ((tid >> 4) & 3) * 4 + (tid >> 6)): the first thread, the last
# thread's last pixel in its second row, the last row of the first row block, the first of the second, one in the middle,
# and one for each (wave, thread row) the others leave out -- together all eight
SINGLE = [(0, 0), (31, 63), (15, 60), (16, 0), (3, 17), (2, 5), (22, 40), (21, 9), (5, 33)]


def _wave_and_thread_row(row):
    """Tile-local row -> (wave, thread row) of the thread of k_bp_bin that holds it."""
    return (row % 16) % 4, row // 16


def _single_pixel_positions(v):
    """One pixel per tile of view v -> [(row, col)] in image coordinates.  The full tiles rotate through SINGLE, the bottom
    tiles take the last image row, the right tiles column 128 + v (over the four views: each of the last four columns)."""
    pos = []
    for i, (ty, tx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        r, c = SINGLE[(i + 4 * v) % len(SINGLE)]
        pos.append((ty * TH + r, tx * TW + c))
    for tx, c in ((0, (0, 63, 17, 60)[v]), (1, (63, 0, 60, 17)[v])):
        pos.append((H - 1, tx * TW + c))
    for ty, r in ((0, (2, 21, 15, 16)[v]), (1, (31, 22, 5, 0)[v])):
        pos.append((ty * TH + r, 2 * TW + v))
    pos.append((H - 1, 2 * TW + v))
    return pos


def _sparse(depth):
    """The views with all but one pixel per tile zeroed; the kept pixel keeps its depth of the scene (7.5 m where that is
    not live)."""
    out = np.zeros_like(depth)
    for v in range(depth.shape[0]):
        for r, c in _single_pixel_positions(v):
            out[v, r, c] = depth[v, r, c] if depth[v, r, c] >= 0.5 else 7.5
    return out


def test_positions_cover_every_wave_row_and_partial_tile():
    """(no GPU work) Over the four views: one pixel per tile; every position of SINGLE in a full tile; every one of the
    eight (wave, thread row) pairs of the kernel's row mapping as the ONLY live lane of a full tile, and again of a tile
    of the 4-pixel-wide column; every one of the last four columns; the last image row."""
    seen, full, right = set(), set(), set()
    for v in range(4):
        pos = _single_pixel_positions(v)
        assert len({(r // TH, c // TW) for r, c in pos}) == 9 == len(pos)
        seen |= {(r % TH, c % TW) for r, c in pos if r < 2 * TH and c < 2 * TW}
        full |= {_wave_and_thread_row(r % TH) for r, c in pos if r < 2 * TH and c < 2 * TW}
        right |= {_wave_and_thread_row(r % TH) for r, c in pos if r < 2 * TH and c >= 2 * TW}
        assert (H - 1, 2 * TW + v) in pos
    every = {(w, t) for w in range(4) for t in range(2)}
    assert seen == set(SINGLE)
    assert full == every and right == every


@pytest.mark.parametrize("key_axis", [1, 2])
def test_single_live_pixel_per_tile_is_never_lost(st, below, key_axis):
    """Maps that are zero except for ONE live pixel per tile, at the lanes whose vote is easiest to lose.  Every one of the
    nine pixels is a voxel of its own (asserted on the oracle's answer), so a lost vote is a lost voxel."""
    depth, cal, masks = below
    sparse = _sparse(depth)
    want = [_bp_oracle(sparse[v], cal[v], masks[v], key_axis) for v in range(4)]
    for v in range(4):
        assert sorted(want[v][0].tolist()) == sorted(r * W + c for r, c in _single_pixel_positions(v)), v
    _assert_oracle(_bp_run(st, sparse, cal, masks, key_axis), want)


DEAD = [0.0, -1.0, 0.0005]              # no depth, a negative one, one below depth_min = 0.001


def test_dead_views_give_no_voxel_and_leave_the_bit_map_zero(st, below):
    """Whole views of 0, of -1 and of 0.0005: no voxel, status 0, and after the binning phases alone the first-pixel bit map
    is all zero (the scratch starts with four counters per view, then 32 bit-map words per tile of 64 x 16 pixels)."""
    _, cal, masks = below
    depth = np.stack([np.full((H, W), d, np.float32) for d in DEAD])
    n_vox, _, _, _, status = _bp_run(st, depth, cal[:3], masks[:3])
    assert status == 0 and not n_vox.any()
    V = 3
    geom, E = st.make_geom()
    table = torch.empty(V * E * st.TABLE_ENTRY_BYTES, dtype=torch.uint8, device=DEV)
    st.bin_table_init(table, V * E)
    cap_vox = 1 << 16
    pw, bw = st.backproject_scratch_words(V, H, W, cap_vox, geom.max_points_per_voxel, geom)
    i32 = lambda n: torch.zeros(n, dtype=torch.int32, device=DEV)
    f64 = lambda n: torch.zeros(n, dtype=torch.float64, device=DEV)
    blk, status = i32(bw), i32(1)
    st.backproject_bin(_t(depth), _t(np.stack([c.record() for c in cal[:3]])), _t(masks[:3]), _t(np.full(V, 4, np.int32)), V, 4,
                       H, W, geom, E, 1, table, i32(pw), blk, cap_vox, i32(V), i32(V * cap_vox), i32(V * cap_vox),
                       f64(V * cap_vox), f64(V * cap_vox), f64(V * cap_vox), status, phases=st.BP_BIN | st.BP_AMB)
    torch.cuda.synchronize()
    bw_view = ((W + 63) // 64) * ((H + 15) // 16) * 32
    head = blk[:4 * V + V * bw_view].cpu().numpy()
    assert int(status.item()) == 0 and not head.any()


def test_dead_views_with_one_live_tile_in_the_middle(st, below):
    """The same three dead maps, each with the middle tile (rows 32 .. 63, columns 64 .. 127) of the scene put back."""
    scene, cal, masks = below
    depth = np.stack([np.full((H, W), d, np.float32) for d in DEAD])
    depth[:, TH:2 * TH, TW:2 * TW] = scene[:3, TH:2 * TH, TW:2 * TW]
    want = [_bp_oracle(depth[v], cal[v], masks[v]) for v in range(3)]
    assert all(len(w[0]) > 100 for w in want)
    _assert_oracle(_bp_run(st, depth, cal[:3], masks[:3]), want)


def test_tiles_live_by_depth_but_kept_nowhere(st, across):
    """Tiles above the horizon filled with a constant 60 m: every pixel passes the depth test and fails z < z_max or
    theta > theta_min (the oracle keeps no pixel of them: the precondition), next to tiles with kept pixels in the same
    view.  View 0: the whole top tile row; view 1: its outer tiles, the middle one empty; views 2 and 3 as generated."""
    depth, cal, masks = across
    depth = depth.copy()
    depth[0, :TH, :] = 60.0
    depth[1, :TH, :] = 0.0
    depth[1, :TH, :TW] = 60.0
    depth[1, :TH, 2 * TW:] = 60.0
    want = [_bp_oracle(depth[v], cal[v], masks[v]) for v in range(4)]
    for v in (0, 1):
        assert len(want[v][0]) > 100 and (want[v][0] // W).min() >= TH, v       # voxels, none of them in the top tile row
    _assert_oracle(_bp_run(st, depth, cal, masks), want)


# a geometry without tier 1: 82 082 theta bins in the window (65 536 or more do not fit the 16 bits a kept pixel carries),
# six phi bins, so the table stays at half a million entries per view
FINE = dict(vsize=(200.0, 2e-5, 1.0), vrange_min=(-100.0, 1.0, -5.0), vgrid=(1, 110000, 10))


@pytest.mark.parametrize("key_axis", [1, 2])
def test_tiles_with_only_undecided_pixels(st, below, key_axis):
    """Under a geometry for which tier 1 decides nothing (asserted with the classification self-test: kept == 0,
    undecided > 0) every live pixel reaches the table through the lists of undecided pixels and the tier-2 kernel: a
    tile without a kept pixel still has work.  A sparse map (one live pixel per tile) and a dense view."""
    depth, cal, masks = below
    geom, _ = st.make_geom(**FINE)
    assert geom.t_n >= 1 << 16
    r = st.selftest_classify(cal[0].record(), H, W, geom, key_axis, 100_000, seed=5, d_lo=0.5, d_hi=95.0)
    assert r["tried"] == 100_000 and r["kept"] == 0 and r["undecided"] > 0 and r["wrong"] == 0, r
    d = np.stack([_sparse(depth)[0], depth[0]])
    c, m = [cal[0], cal[0]], np.stack([masks[0], masks[0]])
    want = [_bp_oracle(d[v], c[v], m[v], key_axis, FINE) for v in range(2)]
    assert len(want[0][0]) == 9 and len(want[1][0]) > 1000
    _assert_oracle(_bp_run(st, d, c, m, key_axis, geom_kw=FINE), want)


def test_one_view_at_bench_size(st):
    """One 900 x 1600 view of the benchmark's scenes: a real horizon crosses tile rows, so empty tiles, tiles that are
    live but kept nowhere and full tiles sit side by side."""
    from dfu3d_amd import synth
    s = synth.make_scene(0, H=900, W=1600, M=8, cams=1, dense=True, k_min=30, k_max=40)
    depth, masks = s.depth.numpy(), s.masks.numpy()
    want = [_bp_oracle(depth[0], s.calibs[0], masks[0])]
    assert 1000 < len(want[0][0]) < 1 << 18
    _assert_oracle(_bp_run(st, depth, s.calibs, masks, cap_vox=1 << 18), want)
