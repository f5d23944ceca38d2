"""The hard-voxel stage without a GPU: the restatement of its rule (tests/hard_voxel_ref.py) against the oracle's
orc_voxelize where float32 and float64 cells agree exactly, the agreement of csrc/dfu3d_hvox.h with its binding, host-side
argument validation before any launch, the `transform_points_to_voxels` entry of DataProcessor, and MeanVFE against
the reference's recorded output (golden G23)."""
import ctypes
import glob
import importlib
import os

import numpy as np
import pytest

from dfu3d_amd import _build, _lib, _lib_hvox
from tests import hard_voxel_ref as H

SYMBOLS = ['dfu3d_hard_voxels', 'dfu3d_hvox_scratch_bytes', 'dfu3d_hvox_version']
POINTERS = ('points', 'point_cnt', 'range_min', 'voxel_size', 'grid', 'scratch', 'voxel_cnt', 'n_voxels', 'voxel_coords',
            'voxel_num_points', 'voxels', 'voxel_mean', 'point_voxel', 'status')
HOST = ('range_min', 'voxel_size', 'grid')                     # read on the host during the call
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g23_hard_voxel.npz")
RANGE = [0.0, -40.0, -3.0, 70.4, 40.0, 1.0]
MASK = {'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True}


# ---- the restatement against the oracle ---------------------------------------------------------------------------------
def oracle_voxelize(xyz, vs, rmin, grid, T, max_voxels):
    """orc_voxelize (oracle a8) on float64 copies -> (voxel of every stored row or -1, n_vox, counts, cells)."""
    from oracle import penet_oracle as O
    n = len(xyz)
    coords = np.ascontiguousarray(xyz, np.float64)
    g = np.array(grid, np.int32)
    tab = np.full(int(g[0]) * int(g[1]) * int(g[2]), -1, np.int32)
    vox_of_pt = np.empty(n, np.int32)
    cap = max(min(n, max_voxels), 1)
    cnt, cell = np.empty(cap, np.int32), np.empty(cap, np.int64)
    nv = O._lib().orc_voxelize(O._p(coords), ctypes.c_int64(3), ctypes.c_int64(n), O._p(np.array(vs, np.float64)),
                               O._p(np.array(rmin, np.float64)), O._p(g), ctypes.c_int32(T), ctypes.c_int32(max_voxels),
                               O._p(tab), O._p(vox_of_pt), O._p(cnt), O._p(cell))
    assert (tab == -1).all()
    return vox_of_pt, int(nv), cnt[:nv], cell[:nv]


@pytest.mark.parametrize("T,max_voxels", [(3, 10 ** 6), (1, 10 ** 6), (4, 25), (100, 1)])
def test_the_restatement_against_the_oracle_where_both_are_exact(T, max_voxels):
    """Voxel sizes that are powers of two, range minima that are multiples of them, coordinates that are multiples of a
    quarter voxel: the float32 and the float64 cell computations are both exact, so the two sequential rules must agree
    on the voxel of every stored row, on the counts and on the order."""
    rng = np.random.default_rng(80)
    vs, rmin, grid = (0.25, 0.5, 2.0), (-2.0, 1.5, -4.0), (12, 9, 3)
    n = 900
    quarter = np.stack([rng.integers(-6, 4 * grid[j] + 6, n) for j in range(3)], 1)     # some rows outside on every side
    xyz = (np.array(rmin) + quarter * (np.array(vs) / 4)).astype(np.float32)
    assert np.array_equal(xyz.astype(np.float64), np.array(rmin) + quarter * (np.array(vs) / 4))
    pts = np.concatenate([np.zeros((n, 1), np.float32), xyz, rng.uniform(0, 1, (n, 1)).astype(np.float32)], 1)
    got = H.hard_voxels(pts, [n], rmin, vs, grid, T, max_voxels)
    vox_of_pt, nv, cnt, cell = oracle_voxelize(xyz, vs, rmin, grid, T, max_voxels)
    assert int(got['n_voxels'][0]) == nv == int(got['voxel_cnt'][0]) and nv == min(max_voxels, nv) and nv > 0
    assert np.array_equal(got['point_voxel'], vox_of_pt) and (vox_of_pt == -1).any() and (vox_of_pt >= 0).any()
    assert np.array_equal(got['voxel_num_points'][:nv], cnt) and cnt.max() == min(T, cnt.max())
    co = got['voxel_coords'][:nv]                                 # [b, z, y, x]; the oracle's cell is (x * gy + y) * gz + z
    assert np.array_equal((co[:, 3].astype(np.int64) * grid[1] + co[:, 2]) * grid[2] + co[:, 1], cell) and not co[:, 0].any()
    inside, c, _ = H.cells(xyz, rmin, vs, grid)
    assert np.array_equal(c[inside], np.floor(quarter[inside] / 4).astype(np.int64))


def test_the_restatement_on_a_batch_and_the_mean():
    f = np.float32
    # two scenes over the same two cells; T = 2: the third row of a cell is dropped
    rows = np.array([[9, 0.1, 0.1, 0.1, 1.5], [9, 1.1, 0.1, 0.1, -0.0], [9, 0.2, 0.2, 0.2, 2.5], [9, 0.3, 0.3, 0.3, 100.0],
                     [9, 0.4, 0.1, 0.1, 7.0], [9, np.nan, 0, 0, 1], [9, 5.0, 0, 0, 1]], f)
    got = H.hard_voxels(rows, [4, 3], (0, 0, 0), (1, 1, 1), (2, 2, 2), 2, 5)
    assert got['voxel_cnt'].tolist() == [2, 1] and got['n_voxels'].tolist() == [3] and got['status'].tolist() == [H.BAD_POINT]
    assert got['point_voxel'].tolist() == [0, 1, 0, -1, 2, -1, -1] and len(got['voxel_coords']) == 7
    assert got['voxel_coords'][:4].tolist() == [[0, 0, 0, 0], [0, 0, 0, 1], [1, 0, 0, 0], [-1] * 4]
    assert got['voxel_num_points'].tolist() == [2, 1, 1, 0, 0, 0, 0]
    m = got['voxel_mean']
    assert m[0].tolist() == [f(f(0.1) + f(0.2)) / f(2), f(f(0.1) + f(0.2)) / f(2), f(f(0.1) + f(0.2)) / f(2), 2.0]
    assert m[1, 3] == 0 and not np.signbit(m[1, 3]) and np.signbit(got['voxels'][1, 0, 3]) and not m[3:].any()
    assert H.hard_voxels(rows, [4, -1, 9], (0, 0, 0), (1, 1, 1), (2, 2, 2), 2, 5)['status'][0] == H.BAD_POINT | H.BAD_COUNT
    assert H.hard_voxels(rows, [4, 3], (0, 0, 0), (1, 1, 1), (2, 2, 2), 2, 5, out_cols=3)['voxels'].shape == (7, 2, 3)


# ---- header, binding, validation ---------------------------------------------------------------------------------------------
def test_header_and_binding_agree():
    assert _lib_hvox.HEADER == os.path.join(_build.CSRC, "dfu3d_hvox.h") and _lib_hvox.HEADER in _build._deps()
    assert "dfu3d_hvox.h" not in os.listdir(_build.INCLUDE)
    assert _lib_hvox.header_symbols() == SYMBOLS
    L = _lib_hvox.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert L.dfu3d_hvox_version() == _lib_hvox.header_version() == 1
    K = _lib_hvox.CONSTANTS
    assert all(k.startswith("DFU3D_HVOX_") for k in K)
    assert K == {'DFU3D_HVOX_VERSION': 1, 'DFU3D_HVOX_LAUNCHES': 7, 'DFU3D_HVOX_MAX_POINTS': 128,
                 'DFU3D_HVOX_MAX_BATCH': 65535, 'DFU3D_HVOX_MAX_ELEMS': 2 ** 31 - 1, 'DFU3D_HVOX_KEY_BITS': 62,
                 'DFU3D_HVOX_TABLE_PER_ROW': 2, 'DFU3D_HVOX_ST_BAD_POINT': 1, 'DFU3D_HVOX_ST_BAD_COUNT': 2,
                 'DFU3D_HVOX_ROW_THREADS': 1024, 'DFU3D_HVOX_OUT_THREADS': 256}
    assert K['DFU3D_HVOX_MAX_POINTS'] >= 100 and (H.BAD_POINT, H.BAD_COUNT) == (1, 2)
    res, args = _lib_hvox.SIGNATURES['dfu3d_hard_voxels']
    assert res is ctypes.c_int32 and len(args) == 22 and args[-1] is ctypes.c_void_p
    assert args[2:5] == [ctypes.c_int32] * 3 and args[8:11] == [ctypes.c_int32] * 3 and args[12] is ctypes.c_size_t
    assert ctypes.c_float not in args and args.count(ctypes.c_void_p) == 15
    assert _lib_hvox.SIGNATURES['dfu3d_hvox_scratch_bytes'] == (ctypes.c_size_t, [ctypes.c_int32] * 2)   # no grid enters
    assert _lib_hvox.SIGNATURES['dfu3d_hvox_version'] == (ctypes.c_int32, [])
    others = [os.path.basename(p)[:-3] for p in glob.glob(os.path.join(os.path.dirname(_lib.__file__), "_lib*.py"))]
    assert "_lib_hvox" in others and "_lib_smp" in others and "_lib" in others
    for name in others:
        if name != "_lib_hvox":
            mod = importlib.import_module("dfu3d_amd." + name)
            assert not set(_lib_hvox.SIGNATURES) & set(mod.SIGNATURES), name
            assert not set(K) & set(mod.CONSTANTS), name
    own = open(_lib_hvox.HEADER).read()
    for prefix in ('dfu3d_vox', 'dfu3d_vfe', 'dfu3d_head', 'dfu3d_post', 'dfu3d_aug', 'dfu3d_bev', 'dfu3d_opt',
                   'dfu3d_ingest', 'dfu3d_pn2', 'dfu3d_roi', 'dfu3d_tgt', 'dfu3d_prop', 'dfu3d_smp'):
        assert prefix not in own and prefix.upper() not in own, prefix
    from dfu3d_amd import hard_voxel_ops as ops
    assert (ops.LAUNCHES, ops.MAX_POINTS) == (7, 128) and ops.status_message(0) == "ok"
    assert "non-finite" in ops.status_message(1) and "point_cnt" in ops.status_message(3)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
    Fake.dfu3d_hvox_version = object()
    with pytest.raises(_lib.Dfu3dError, match="fake.so does not export dfu3d_hard_voxels, dfu3d_hvox_scratch_bytes"):
        _lib_hvox.bind(Fake())


def _call(L, B=2, R=500, C=4, T=5, mv=100, oc=4, nbytes=None, rmin=(0.0, -40.0, -3.0), vs=(0.05, 0.05, 0.1),
          dims=(1408, 1600, 40), **ptr):
    p = {name: ctypes.c_void_p(16 * (k + 1)) for k, name in enumerate(POINTERS)}      # addresses no call may touch
    keep = ((ctypes.c_float * 3)(*rmin), (ctypes.c_float * 3)(*vs), (ctypes.c_int32 * 3)(*dims))
    p.update({name: ctypes.cast(a, ctypes.c_void_p) for name, a in zip(HOST, keep)})
    p.update(ptr)
    if nbytes is None:
        nbytes = L.dfu3d_hvox_scratch_bytes(B, R) or 16
    return L.dfu3d_hard_voxels(p['points'], p['point_cnt'], B, R, C, p['range_min'], p['voxel_size'], p['grid'], T, mv, oc,
                               p['scratch'], nbytes, p['voxel_cnt'], p['n_voxels'], p['voxel_coords'],
                               p['voxel_num_points'], p['voxels'], p['voxel_mean'], p['point_voxel'], p['status'], None)


def test_bad_arguments_return_before_any_launch():
    """Every call below passes device pointers no kernel may touch: a launch would fault (or, without a GPU, fail with
    DFU3D_ELAUNCH); each must come back with the validation's own code."""
    L = _lib_hvox.lib()
    OK, EINVAL, ERANGE = (_lib.CONSTANTS[k] for k in ("DFU3D_OK", "DFU3D_EINVAL", "DFU3D_ERANGE"))
    K = _lib_hvox.CONSTANTS
    for name in POINTERS:
        if name not in ('voxels', 'voxel_mean'):
            assert _call(L, **{name: None}) == EINVAL, name
    assert _call(L, voxels=None, voxel_mean=None) == EINVAL         # both output blocks null
    assert _call(L, B=-1) == EINVAL and _call(L, R=-1) == EINVAL
    assert _call(L, T=0) == EINVAL and _call(L, T=-4) == EINVAL and _call(L, mv=0) == EINVAL and _call(L, mv=-1) == EINVAL
    assert _call(L, C=2, oc=2) == EINVAL and _call(L, C=0, oc=0) == EINVAL and _call(L, C=-1) == EINVAL
    assert _call(L, oc=2) == EINVAL and _call(L, oc=5) == EINVAL and _call(L, C=6, oc=7) == EINVAL and _call(L, oc=-1) == EINVAL
    for j in range(3):
        def at(base, v):
            return tuple(v if k == j else x for k, x in enumerate(base))
        assert _call(L, dims=at((8, 8, 8), 0)) == EINVAL and _call(L, dims=at((8, 8, 8), -5)) == EINVAL
        for v in (0.0, -0.1, float('nan'), float('inf')):
            assert _call(L, vs=at((0.1, 0.1, 0.1), v)) == EINVAL, (j, v)
        for v in (float('nan'), float('-inf')):
            assert _call(L, rmin=at((0.0, 0.0, 0.0), v)) == EINVAL, (j, v)
    assert _call(L, scratch=ctypes.c_void_p(24)) == EINVAL                        # not on 16 bytes
    need = L.dfu3d_hvox_scratch_bytes(2, 500)
    assert need > 0 and _call(L, nbytes=need - 1) == EINVAL and _call(L, nbytes=0) == EINVAL
    # nothing to do: no launch, and the scratch is not looked at
    assert _call(L, B=0) == OK and _call(L, B=0, R=0, nbytes=0) == OK
    assert _call(L, B=0, R=0, points=None, point_voxel=None, voxel_coords=None, voxel_num_points=None) == OK
    assert _call(L, T=K['DFU3D_HVOX_MAX_POINTS'] + 1) == ERANGE
    assert _call(L, B=K['DFU3D_HVOX_MAX_BATCH'] + 1, nbytes=1 << 30) == ERANGE
    assert _call(L, B=1, dims=(2 ** 21, 2 ** 21, 2 ** 20)) == ERANGE              # 2^62 cells
    assert _call(L, B=3, dims=(2 ** 21, 2 ** 20, 2 ** 20)) == ERANGE              # 3 * 2^61
    assert _call(L, B=65535, dims=(2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1), nbytes=1 << 40) == ERANGE   # no 64-bit wrap-around
    assert _call(L, R=2 ** 31 - 1, nbytes=1 << 40) == ERANGE                      # R * (1 + C)
    assert _call(L, R=2 ** 29, C=3, oc=3, nbytes=1 << 40) == ERANGE
    assert _call(L, R=2 ** 28, C=3, oc=3, T=4, mv=2 ** 28, nbytes=1 << 40) == ERANGE      # V_cap * T * out_cols
    # an out-of-range size wins over what is empty, an invalid one over both
    assert _call(L, B=0, T=K['DFU3D_HVOX_MAX_POINTS'] + 1) == ERANGE and _call(L, B=0, oc=2) == EINVAL


def test_scratch_bytes_grow_with_the_rows_only():
    L = _lib_hvox.lib()
    K = _lib_hvox.CONSTANTS
    for bad in ((-1, 64), (2, -1), (K['DFU3D_HVOX_MAX_BATCH'] + 1, 64), (0, 64)):
        assert L.dfu3d_hvox_scratch_bytes(*bad) == 0, bad
    assert len(_lib_hvox.SIGNATURES['dfu3d_hvox_scratch_bytes'][1]) == 2           # B and R: no grid to depend on
    by_rows = [L.dfu3d_hvox_scratch_bytes(3, R) for R in (0, 1, 16, 17, 100000, 2 ** 29, 2 ** 31 - 1)]
    assert all(a <= b for a, b in zip(by_rows, by_rows[1:])) and by_rows[0] > 0 and by_rows[3] < by_rows[4] < by_rows[-1]
    assert all(s % 16 == 0 for s in by_rows) and by_rows[-1] > 2 ** 32             # no 32-bit wrap-around
    # the table: the power of two of entries at or above 2 R, 20 bytes each; four words per row; the rest is small
    for R in (1000, 4096, 70001):
        entries = 1 << (2 * R - 1).bit_length()
        assert 20 * entries + 16 * R <= L.dfu3d_hvox_scratch_bytes(4, R) <= 20 * entries + 16 * R + 8 * (R // 1024) + 512
        assert entries >= K['DFU3D_HVOX_TABLE_PER_ROW'] * R
    by_b = [L.dfu3d_hvox_scratch_bytes(B, 5000) for B in (1, 2, 100, 65535)]
    assert all(a <= b for a, b in zip(by_b, by_b[1:])) and by_b[-1] - by_b[0] <= 65535 * 12 + 64


# ---- DataProcessor ---------------------------------------------------------------------------------------------------------
def entry(**over):
    cfg = {'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': [0.05, 0.05, 0.1], 'MAX_POINTS_PER_VOXEL': 5,
           'MAX_NUMBER_OF_VOXELS': {'train': 16000, 'test': 40000}}
    cfg.update(over)
    return cfg


def test_data_processor_construction():
    from dfu3d_amd.pcdet_kitti.data_processor import DataProcessor
    # the two dataset configurations of the nuScenes-to-KITTI files, as KittiDataset hands their range over (float32)
    n2k = np.array([0, -54.0, -5.0, 54.0, 54.0, 3.0], np.float32)
    cp = entry(VOXEL_SIZE=[0.075, 0.075, 0.2], MAX_POINTS_PER_VOXEL=10, MAX_NUMBER_OF_VOXELS={'train': 120000, 'test': 160000})
    pr = entry(VOXEL_SIZE=[0.1, 0.1, 0.2], MAX_POINTS_PER_VOXEL=10, MAX_NUMBER_OF_VOXELS={'train': 60000, 'test': 60000})
    p = DataProcessor([MASK, cp], n2k, True, 4, device="cpu")
    assert list(p.grid_size) == [720, 1440, 40] and p.grid_size.dtype == np.int64 and p.voxel_size == [0.075, 0.075, 0.2]
    assert p.voxel_config() == {'voxel_size': [0.075, 0.075, 0.2], 'grid_size': [720, 1440, 40], 'max_points': 10,
                                'max_voxels': 120000}
    t = DataProcessor([MASK, cp], n2k, False, 4, device="cpu")
    assert t.voxel_config()['max_voxels'] == 160000 and t.sample_count() is None
    assert list(DataProcessor([MASK, pr], n2k, True, 4, device="cpu").grid_size) == [540, 1080, 40]
    # KITTI's own: 90 million cells
    k = DataProcessor([MASK, entry()], np.array(RANGE, np.float32), True, 4, device="cpu")
    assert list(k.grid_size) == [1408, 1600, 40] and k.voxel_config()['max_voxels'] == 16000
    q = DataProcessor([MASK, entry(VOXEL_SIZE=[0.1, 0.1, 0.15])], np.array(RANGE, np.float32), True, 4, device="cpu")
    expect = np.round((np.array(RANGE, np.float32)[3:6] - np.array(RANGE, np.float32)[0:3]) / np.array([0.1, 0.1, 0.15]))
    assert list(q.grid_size) == expect.astype(np.int64).tolist() == [704, 800, 27]
    assert DataProcessor([MASK], RANGE, True, 4, device="cpu").voxel_config() is None
    for bad in (entry(DOUBLE_FLIP=True), {k: v for k, v in entry().items() if k != 'MAX_POINTS_PER_VOXEL'},
                {k: v for k, v in entry().items() if k != 'MAX_NUMBER_OF_VOXELS'},
                {'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': [0.1, 0.1, 0.1]}):
        with pytest.raises(NotImplementedError):
            DataProcessor([MASK, bad], RANGE, True, 4, device="cpu")
    with pytest.raises(_lib.Dfu3dError, match="MAX_POINTS_PER_VOXEL"):
        DataProcessor([MASK, entry(MAX_POINTS_PER_VOXEL=129)], RANGE, True, 4, device="cpu")


# ---- MeanVFE against the reference -------------------------------------------------------------------------------------------
def test_mean_vfe_against_the_reference():
    """Golden G23: the reference's MeanVFE on the restatement's voxels.  Tolerance per element T * 2^-23 * sum|x_k| /
    max(n, 1): both sides are float32 sums of the same <= T terms in some order, each within (T - 1) * 2^-24 * sum|x| of the
    exact sum, followed by one division."""
    import torch
    from dfu3d_amd.pcdet_kitti.mean_vfe import MeanVFE
    g = np.load(GOLDEN)
    T = int(g['max_points'])
    out = H.hard_voxels(g['points'], g['point_cnt'], g['range_min'], g['voxel_size'], g['grid'], T, int(g['max_voxels']))
    nv = int(out['n_voxels'][0])
    voxels, num, want = g['voxels'], g['voxel_num_points'], g['voxel_features']
    assert voxels.shape == (nv + 1, T, 4) and np.array_equal(voxels[:nv], out['voxels'][:nv]) and num[-1] == 0
    assert np.array_equal(num[:nv], out['voxel_num_points'][:nv]) and num.max() == T and (num == 1).any()
    vfe = MeanVFE({}, 4)
    assert vfe.get_output_feature_dim() == 4 and not list(vfe.parameters())
    batch = vfe({'voxels': torch.from_numpy(voxels), 'voxel_num_points': torch.from_numpy(num)})
    got = batch['voxel_features'].numpy()
    assert got.dtype == np.float32 and got.shape == want.shape == (nv + 1, 4)
    assert got.tobytes() == H.mean(voxels, num).tobytes()          # the stage's rule, bit for bit
    assert got[:nv].tobytes() == out['voxel_mean'][:nv].tobytes()
    tol = T * 2.0 ** -23 * np.abs(voxels.astype(np.float64)).sum(1) / np.maximum(num, 1)[:, None]
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol).all()
    assert not got[-1].any() and not np.signbit(got[-1]).any()      # the voxel with 0 points
    lone = np.flatnonzero((num == 1) & np.signbit(voxels[:, 0, 3]))
    assert len(lone) == 1 and got[lone[0], 3] == 0                  # the single -0.0
    # only voxel_features in the batch: unchanged, the same object
    feats = torch.from_numpy(want.copy())
    assert vfe({'voxel_features': feats})['voxel_features'] is feats
    with pytest.raises(_lib.Dfu3dError):
        vfe({'points': feats})
