"""The hard-voxel stage on the GPU (csrc/hardvoxel_stage.hip) against tests/hard_voxel_ref.py, the sequential restatement
of THE RULE and THE MEAN of csrc/dfu3d_hvox.h: every output of every case is compared bit for bit, the -1 / 0 tails and
the status word included, in the three output forms (voxels, mean, both).  Then the layers above it: prepare_batch,
MeanVFE, and a KittiDataset whose processor list ends in transform_points_to_voxels."""
import functools

import numpy as np
import pytest

from tests import hard_voxel_ref as H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
KEYS = ("voxel_cnt", "n_voxels", "voxel_coords", "voxel_num_points", "voxels", "voxel_mean", "point_voxel", "status")
# a small grid for most cases: 0.5 m cells (exact in float32), 16 x 12 x 4 of them
RMIN, VS, GRID = (-4.0, -3.0, -1.0), (0.5, 0.5, 0.5), (16, 12, 4)


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def block(scenes, tail=0):
    """Scenes (n_b, C) -> points (sum n + tail, 1 + C) with the scene index in column 0 and point_cnt int32 (B).  The
    `tail` rows behind the last scene hold NaN and index -1: the stage never reads them."""
    C = scenes[0].shape[1]
    rows = [np.concatenate([np.full((len(s), 1), b, f32), np.asarray(s, f32)], 1) for b, s in enumerate(scenes)]
    pad = np.full((tail, 1 + C), np.nan, f32)
    pad[:, 0] = -1
    return np.concatenate(rows + [pad], 0), np.array([len(s) for s in scenes], np.int32)


def in_cells(rng, cell, C=4, rmin=RMIN, vs=VS):
    """One row inside each of the cells (n, 3) [x, y, z], at a random place of it, the other columns random."""
    cell = np.asarray(cell, np.float64).reshape(-1, 3)
    xyz = np.asarray(rmin) + (cell + rng.uniform(0.1, 0.9, cell.shape)) * np.asarray(vs)
    return np.concatenate([xyz, rng.uniform(-1, 1, (len(cell), C - 3))], 1).astype(f32)


def run(points, cnt, rmin, vs, grid, T, mv, out_cols=None, form="both"):
    import torch
    from dfu3d_amd import hard_voxel_ops as ops
    out = ops.hard_voxels(cu(points), cu(cnt), list(rmin) + [0, 0, 0], vs, grid, T, mv, out_cols=out_cols,
                          want_voxels=form != "mean", want_mean=form != "voxels")
    torch.cuda.synchronize()
    return {k: getattr(out, k).cpu().numpy() for k in KEYS if getattr(out, k) is not None}


def compare(got, exp, what=""):
    for k in KEYS:
        if k in got:
            assert same_bits(got[k], exp[k]), (what, k, got[k].shape, exp[k].shape,
                                               np.argwhere(got[k].reshape(-1).view(np.uint32)
                                                           != exp[k].reshape(-1).view(np.uint32))[:8].tolist()
                                               if got[k].shape == exp[k].shape else None)


def check(points, cnt, rmin=RMIN, vs=VS, grid=GRID, T=5, mv=1000, out_cols=None, forms=("both", "voxels", "mean"),
          what=""):
    """The stage in every form against the restatement -> the restatement's outputs."""
    exp = H.hard_voxels(points, cnt, rmin, vs, grid, T, mv, out_cols)
    for form in forms:
        got = run(points, cnt, rmin, vs, grid, T, mv, out_cols, form)
        assert ("voxels" in got) == (form != "mean") and ("voxel_mean" in got) == (form != "voxels")
        compare(got, exp, (what, form))
    return exp


# ---- boundaries -------------------------------------------------------------------------------------------------------
def rounds_up_to_the_grid(vs=0.075):
    """(p, grid): a float32 p >= 0 with p / fl32(vs) < grid exactly but fl32(p / fl32(vs)) == grid."""
    v = f32(vs)
    for grid in range(1400, 1500):
        p = f32(grid * float(v))
        for _ in range(8):
            p = np.nextafter(p, f32(0.0))
            if float(p) / float(v) < grid and np.divide(p, v, dtype=f32) == f32(grid):
                return p, grid
    return None


def test_boundaries():
    rng = np.random.default_rng(1)
    below = lambda v: np.nextafter(f32(v), f32(-np.inf))                               # noqa: E731
    hi = [RMIN[j] + VS[j] * GRID[j] for j in range(3)]
    rows = [list(RMIN), [below(RMIN[0]), RMIN[1], RMIN[2]], [RMIN[0], below(RMIN[1]), RMIN[2]],
            [RMIN[0], RMIN[1], below(RMIN[2])], [hi[0], 0, 0], [0, hi[1], 0], [0, 0, hi[2]],
            [below(hi[0]), below(hi[1]), below(hi[2])], list(RMIN), [np.nan, 0, 0], [0, np.inf, 0], [0, 0, -np.inf],
            [1.25, 0.25, 0.25], [-0.0, -0.0, -0.0],
            [float(below(VS[j] * GRID[j])) + RMIN[j] for j in range(3)]]
    p = np.concatenate([np.array(rows, f32), rng.uniform(-1, 1, (len(rows), 2)).astype(f32)], 1)
    p[0, 3:] = -0.0                                              # -0.0 features: copied bit for bit; the mean adds them to +0.0
    p[8, 3] = -0.0
    exp = check(*block([p]))
    assert int(exp["status"][0]) == H.BAD_POINT and int(exp["n_voxels"][0]) == 4
    # row 7, the float32 just below the upper bound on every axis, is OUT: p - range_min rounds up to the extent.  Row 14
    # is the largest row that is inside: its difference is the float32 just below the extent, and exact
    assert exp["point_voxel"].tolist() == [0, -1, -1, -1, -1, -1, -1, -1, 0, -1, -1, -1, 1, 2, 3]
    assert exp["voxel_coords"][3].tolist() == [0, GRID[2] - 1, GRID[1] - 1, GRID[0] - 1]
    assert np.signbit(exp["voxels"][0, 0, 3]) and not np.signbit(exp["voxel_mean"][0, 3])
    # the quotient that rounds up to the grid: OUT by THE RULE though the exact quotient is inside
    found = rounds_up_to_the_grid()
    assert found is not None
    edge, g = found
    q = np.array([[edge, 0.1, 0.1, 0.5], [np.nextafter(edge, f32(0)), 0.1, 0.1, 0.5], [0.1, edge, 0.1, 0.5]], f32)
    exp = check(*block([q]), rmin=(0.0, 0.0, 0.0), vs=(0.075, 0.075, 0.2), grid=(g, g, 40))
    assert exp["point_voxel"].tolist()[0] == -1 and exp["point_voxel"].tolist()[2] == -1 and int(exp["status"][0]) == 0


# ---- the voxel cap ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mv", [7, 1])
def test_the_voxel_cap(mv):
    rng = np.random.default_rng(2)
    order = rng.permutation(40)
    cell = np.stack([order % 16, order // 16 + 2, np.ones(40, int)], 1)
    first = in_cells(rng, cell)                                   # 40 cells, once each
    later = in_cells(rng, cell[rng.integers(0, 40, 120)])         # then 120 rows that fall into them
    exp = check(*block([np.concatenate([first, later])]), mv=mv, T=4)
    pv = exp["point_voxel"]
    assert int(exp["n_voxels"][0]) == mv and (pv[mv:40] == -1).all() and (pv[:mv] == np.arange(mv)).all()
    assert (pv[40:] >= 0).any() and exp["voxel_num_points"][:mv].max() > 1   # rows behind the cap still join the first cells


# ---- the slot cap -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crowded(n_hot, n_other, seed):
    """One cell of n_hot rows interleaved with n_other rows in other cells."""
    rng = np.random.default_rng(seed)
    hot = rng.permutation(n_hot + n_other) < n_hot
    cell = np.stack([rng.integers(0, 16, len(hot)), rng.integers(0, 12, len(hot)), rng.integers(0, 3, len(hot))], 1)
    cell[hot] = (5, 7, 3)
    return block([in_cells(rng, cell)])


@pytest.mark.parametrize("T,n_hot,n_other", [(3, 200, 500), (5, 5000, 0), (5, 5000, 301), (1, 200, 500), (100, 200, 500),
                                             (100, 5000, 777), (128, 300, 100)])
def test_the_slot_cap(T, n_hot, n_other):
    exp = check(*crowded(n_hot, n_other, 3), T=T)
    assert exp["voxel_num_points"].max() == min(T, n_hot)


# ---- batch ------------------------------------------------------------------------------------------------------------
def test_batch_same_cells_empty_scene_all_out_scene():
    rng = np.random.default_rng(4)
    cell = np.stack([rng.integers(0, 16, 300), rng.integers(0, 12, 300), rng.integers(0, 4, 300)], 1)
    a, b, c = in_cells(rng, cell), in_cells(rng, cell), in_cells(rng, cell)
    out = in_cells(rng, cell) + f32(100.0)
    exp = check(*block([a, np.zeros((0, 4), f32), b, out, c], tail=29), mv=50)
    assert exp["voxel_cnt"].tolist() == [50, 0, 50, 0, 50] and int(exp["status"][0]) == 0
    co = exp["voxel_coords"]
    assert (co[:50, 1:] == co[50:100, 1:]).all() and co[:150, 0].tolist() == [0] * 50 + [2] * 50 + [4] * 50
    assert (co[150:] == -1).all() and len(co) == 250
    one = check(*block([a]), mv=1000)                             # B = 1
    assert int(one["n_voxels"][0]) == len({tuple(r) for r in cell.tolist()})


def test_many_scenes():
    rng = np.random.default_rng(5)
    scenes = [in_cells(rng, np.stack([rng.integers(0, 16, n), rng.integers(0, 12, n), rng.integers(0, 4, n)], 1))
              for n in rng.integers(0, 40, 1500)]
    check(*block(scenes), mv=9, T=2, forms=("both",))


# ---- length and load --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def long_scene():
    """70 001 rows: the first 40 000 in 40 000 distinct cells of a 256 x 256 x 4 grid, the rest falling into them."""
    rng = np.random.default_rng(6)
    ids = rng.permutation(256 * 256 * 4)[:40000]
    ids = np.concatenate([ids, ids[rng.integers(0, 40000, 30001)]])
    cell = np.stack([ids % 256, (ids // 256) % 256, ids // 65536], 1)
    return block([in_cells(rng, cell, rmin=(0, 0, 0), vs=(0.25, 0.25, 0.25))])


@pytest.mark.parametrize("mv", [120000, 30000])
def test_a_long_scene_across_workgroups(mv):
    exp = check(*long_scene(), rmin=(0, 0, 0), vs=(0.25, 0.25, 0.25), grid=(256, 256, 4), mv=mv, T=3)
    assert int(exp["n_voxels"][0]) == min(mv, 40000)


def test_the_table_at_its_maximum_load():
    """R = 4096 rows in 4096 distinct cells: the table has 2 R entries, every second one taken."""
    rng = np.random.default_rng(7)
    ids = rng.permutation(64 * 64 * 2)[:4096]
    cell = np.stack([ids % 64, (ids // 64) % 64, ids // 4096], 1)
    p, cnt = block([in_cells(rng, cell[:1000]), in_cells(rng, cell[1000:])])
    exp = check(p, cnt, grid=(64, 64, 2), mv=4096)
    assert int(exp["n_voxels"][0]) == 4096


def test_a_grid_beyond_31_bits_of_cells():
    rng = np.random.default_rng(8)
    grid = (2048, 2048, 1024)
    corner = np.array([[2047, 2047, 1023]] * 7 + [[2047, 2047, 1022], [0, 0, 0], [2047, 0, 1023]])
    p = in_cells(rng, corner, rmin=(0, 0, 0), vs=(0.5, 0.5, 0.5))
    exp = check(*block([p, p[::-1]]), rmin=(0, 0, 0), vs=(0.5, 0.5, 0.5), grid=grid, T=4)
    assert exp["voxel_coords"][0].tolist() == [0, 1023, 2047, 2047] and exp["voxel_num_points"][0] == 4
    assert int(exp["n_voxels"][0]) == 8


@pytest.mark.parametrize("C,oc", [(4, 3), (6, 4), (3, 3), (7, 7)])
def test_out_cols(C, oc):
    rng = np.random.default_rng(9)
    cell = np.stack([rng.integers(0, 16, 700), rng.integers(0, 12, 700), rng.integers(0, 4, 700)], 1)
    exp = check(*block([in_cells(rng, cell[:300], C), in_cells(rng, cell[300:], C)]), out_cols=oc)
    assert exp["voxels"].shape[2] == oc


def test_bad_counts_set_their_bit_and_read_nothing_outside():
    rng = np.random.default_rng(10)
    cell = np.stack([rng.integers(0, 16, 150), rng.integers(0, 12, 150), rng.integers(0, 4, 150)], 1)
    p, _ = block([in_cells(rng, cell)])
    exp = check(p, np.array([100, -7, 90], np.int32))              # scene 2 is cut at the 50 rows there are
    assert int(exp["status"][0]) == H.BAD_COUNT and exp["voxel_cnt"][1] == 0 and exp["voxel_cnt"][2] > 0
    exp = check(p, np.array([2 ** 31 - 1, 2 ** 31 - 1, 5], np.int32))
    assert int(exp["status"][0]) == H.BAD_COUNT and exp["voxel_cnt"].tolist()[1:] == [0, 0]


def test_guard_bands_poisoned_scratch_and_the_same_bits_twice():
    from dfu3d_amd import hard_voxel_ops as ops
    from tests.test_gpu_guard_bands import both_poisons
    p, cnt = crowded(200, 1500, 11)
    p = np.concatenate([p, np.full((13, p.shape[1]), np.nan, f32)])
    cnt = np.array([700, 0, 1000], np.int32)
    exp = H.hard_voxels(p, cnt, RMIN, VS, GRID, 4, 150, 3)

    def once():
        o = ops.hard_voxels(cu(p), cu(cnt), RMIN, VS, GRID, 4, 150, out_cols=3, want_voxels=True, want_mean=True)
        return tuple(getattr(o, k) for k in KEYS)

    def verify(o):
        compare(dict(zip(KEYS, o)), exp)
    first = both_poisons(once, verify, count=11)                 # 2 uploads, status, 7 outputs, scratch
    again = both_poisons(once, verify, count=11)
    for a, b in zip(first, again):
        assert same_bits(a, b)


def test_launch_count_and_no_host_read(monkeypatch):
    """DFU3D_HVOX_LAUNCHES kernel launches for B = 1 and B = 11 (the build that counts its launches), and no
    synchronising call in the wrapper."""
    import ctypes
    import torch
    from dfu3d_amd import _lib, _lib_hvox, hard_voxel_ops as ops
    rng = np.random.default_rng(12)
    scenes = [in_cells(rng, np.stack([rng.integers(0, 16, n), rng.integers(0, 12, n), rng.integers(0, 4, n)], 1))
              for n in [900] + rng.integers(1, 700, 10).tolist()]
    p, cnt = block(scenes)
    dp, dc = cu(p), cu(cnt)
    ops.hard_voxels(dp, dc, RMIN, VS, GRID, 5, 100)                # library loaded, allocator warm
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = ops.hard_voxels(dp, dc, RMIN, VS, GRID, 5, 100, want_mean=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(out.status.item()) == 0
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib, "_LIB", L)
    monkeypatch.setattr(_lib_hvox, "_BOUND", _lib_hvox.bind(L))
    for B in (1, 11):
        pb, cb = p[:int(cnt[:B].sum())], cnt[:B]
        L.dfu3d_debug_launch_count(1)
        got = ops.hard_voxels(cu(pb), cu(cb), RMIN, VS, GRID, 5, 100, want_mean=True)
        assert int(L.dfu3d_debug_launch_count(1)) == ops.LAUNCHES, B
        torch.cuda.synchronize()
        compare({k: getattr(got, k).cpu().numpy() for k in KEYS}, H.hard_voxels(pb, cb, RMIN, VS, GRID, 5, 100))


# ---- prepare_batch ------------------------------------------------------------------------------------------------------
from tests import world_aug_cases as W  # noqa: E402

VOXEL_ENTRY = dict(NAME='transform_points_to_voxels', VOXEL_SIZE=[0.4, 0.4, 0.5], MAX_POINTS_PER_VOXEL=3,
                   MAX_NUMBER_OF_VOXELS={'train': 150, 'test': 170})


class Cfg(dict):
    __getattr__ = dict.__getitem__


def surface(ci, voxels=True, num_points=None):
    """The augmentor and the processor of configuration ci of tests/world_aug_cases.py, the placeholder entry replaced by
    transform_points_to_voxels (voxels) and a sample_points entry behind the range mask (num_points)."""
    from dfu3d_amd.pcdet_kitti.data_augmentor import DataAugmentor
    from dfu3d_amd.pcdet_kitti.data_processor import DataProcessor
    cfg = W.dataset_cfg(ci, False)
    entries = [Cfg(c) for c in cfg['DATA_PROCESSOR']]
    if voxels:
        entries = [e for e in entries if e['NAME'] != 'transform_points_to_voxels_placeholder'] + [Cfg(VOXEL_ENTRY)]
    if num_points is not None:
        entries.insert(1, Cfg(NAME='sample_points', NUM_POINTS={'train': num_points, 'test': num_points}))
    aug = DataAugmentor('.', Cfg(cfg['DATA_AUGMENTOR']), W.class_names(), device=DEV)
    return aug, DataProcessor(entries, W.pc_range(ci), W.training(ci), 4, device=DEV)


def raw_dicts(ci, scenes):
    out = []
    for s in scenes:
        p, b, names = W.inputs(ci, s)
        out.append({'points': p.copy(), 'gt_boxes': b.copy(), 'gt_names': names.copy()})
    return out


def restated(proc, pts, cnt):
    vc = proc.voxel_config()
    return H.hard_voxels(pts, cnt, np.asarray(proc.point_cloud_range, f32)[:3], vc['voxel_size'], vc['grid_size'],
                         vc['max_points'], vc['max_voxels'], 4)


def host_reads(fn):
    """fn() under torch's synchronisation warnings -> (its result, the number of synchronising calls)."""
    import torch
    import warnings
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            out = fn()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    return out, len([x for x in caught if "synchroniz" in str(x.message)])


def test_prepare_batch_is_collate_then_the_restatement():
    import torch
    from dfu3d_amd.pcdet_kitti.data_augmentor import prepare_batch
    from dfu3d_amd.pcdet_kitti.mean_vfe import MeanVFE
    ci, scenes = 0, [7, 3, 5, 4]                                  # 3000, 64, 1024, 1023 points before the mask
    B = len(scenes)
    aug, plain_proc = surface(ci, voxels=False)
    _, proc = surface(ci)
    assert plain_proc.voxel_config() is None and proc.voxel_config()['max_voxels'] == (150 if W.training(ci) else 170)

    def call(p, **kw):
        np.random.seed(5)
        return prepare_batch(raw_dicts(ci, scenes), aug, p, W.class_names(), training=True, **kw)
    plain = call(plain_proc, as_padded=True)
    pts, cnt = plain['points'].cpu().numpy(), plain['point_cnt'].cpu().numpy()
    exp = restated(proc, pts, cnt)
    nv = int(exp['n_voxels'][0])
    assert exp['voxel_cnt'].max() == proc.voxel_config()['max_voxels'] > exp['voxel_cnt'].min() > 0 and exp['status'][0] == 0
    # the padded form: no host read (after a first call: the processor uploads its range once)
    call(proc, as_padded=True)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pad = call(proc, as_padded=True)
        pad_mean = call(proc, as_padded=True, voxel_features_only=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert same_bits(pad['points'].cpu().numpy(), pts) and 'voxel_features' not in pad and 'voxels' not in pad_mean
    for k in ('voxels', 'voxel_coords', 'voxel_num_points', 'voxel_cnt', 'n_voxels'):
        assert same_bits(pad[k].cpu().numpy(), exp[k]), k
    assert same_bits(pad_mean['voxel_features'].cpu().numpy(), exp['voxel_mean'])
    assert same_bits(pad_mean['voxel_coords'].cpu().numpy(), exp['voxel_coords'])
    assert len(pad['status']) == len(plain['status']) + 1 and all(int(s.item()) == 0 for s in pad['status'])
    assert same_bits(pad['gt_boxes'].cpu().numpy(), plain['gt_boxes'].cpu().numpy())
    # the default form: the one host read, as without the entry; everything cut to n_voxels
    before, reads_before = host_reads(lambda: call(plain_proc))
    cut, reads = host_reads(lambda: call(proc))
    feat, reads_feat = host_reads(lambda: call(proc, voxel_features_only=True))
    assert reads == reads_before == reads_feat == 1
    assert sorted(cut) == sorted(list(before) + ['voxel_cnt', 'voxel_coords', 'voxel_num_points', 'voxels'])
    assert sorted(feat) == sorted(list(before) + ['voxel_cnt', 'voxel_coords', 'voxel_features', 'voxel_num_points'])
    assert same_bits(cut['points'].cpu().numpy(), before['points'].cpu().numpy())
    for k in ('voxels', 'voxel_coords', 'voxel_num_points'):
        assert same_bits(cut[k].cpu().numpy(), exp[k][:nv]) and len(cut[k]) == nv, k
    assert same_bits(cut['voxel_cnt'].cpu().numpy(), exp['voxel_cnt'])
    assert same_bits(feat['voxel_features'].cpu().numpy(), exp['voxel_mean'][:nv])
    # MeanVFE: from the voxels, the bits the stage's mean has; from voxel_features alone, nothing to do
    vfe = MeanVFE({}, 4)
    assert same_bits(vfe(dict(cut))['voxel_features'].cpu().numpy(), exp['voxel_mean'][:nv])
    assert vfe(feat)['voxel_features'] is feat['voxel_features']


def test_prepare_batch_with_a_sample_points_entry():
    import torch
    from dfu3d_amd.pcdet_kitti.data_augmentor import prepare_batch
    ci, scenes, K = 0, [7, 3, 5, 4], 200
    aug, proc = surface(ci, num_points=K)
    assert proc.sample_count() == K
    prepare_batch(raw_dicts(ci, scenes), aug, proc, W.class_names(), training=True)    # (the processor uploads its range once)
    np.random.seed(5)
    torch.manual_seed(9)
    (batch, reads) = host_reads(lambda: prepare_batch(raw_dicts(ci, scenes), aug, proc, W.class_names(), training=True))
    pts = batch['points'].cpu().numpy()
    assert reads == 1 and pts.shape == (4 * K, 5) and batch['point_cnt'].tolist() == [K] * 4
    exp = restated(proc, pts, batch['point_cnt'].cpu().numpy())
    nv = int(exp['n_voxels'][0])
    for k in ('voxels', 'voxel_coords', 'voxel_num_points'):
        assert same_bits(batch[k].cpu().numpy(), exp[k][:nv]), k
    assert same_bits(batch['voxel_cnt'].cpu().numpy(), exp['voxel_cnt'])


def test_prepare_batch_reports_the_stage_status():
    from dfu3d_amd import hard_voxel_ops as ops
    from dfu3d_amd._lib import Dfu3dError
    from dfu3d_amd.pcdet_kitti.data_augmentor import prepare_batch
    from dfu3d_amd.pcdet_kitti.data_processor import DataProcessor
    _, proc = surface(0)
    assert proc.mask_mode() != 0
    bare = DataProcessor([Cfg(VOXEL_ENTRY)], W.pc_range(0), True, 4, device=DEV)        # no range mask in front: the NaN arrives
    d = raw_dicts(0, [3])
    d[0]['points'][5, 1] = np.nan
    pad = prepare_batch(d, None, bare, W.class_names(), training=True, as_padded=True)
    assert int(pad['status'][-1].item()) == ops.BAD_POINT
    with pytest.raises(Dfu3dError, match="transform_points_to_voxels status 1 .a point with a non-finite"):
        prepare_batch(d, None, bare, W.class_names(), training=True)


def test_the_per_scene_forward():
    _, proc = surface(0)
    _, plain = surface(0, voxels=False)
    p, b, names = W.inputs(0, 7)
    d = proc.forward({'points': p.copy(), 'gt_boxes': b.copy(), 'gt_names': names.copy(), 'use_lead_xyz': True})
    kept = plain.forward({'points': p.copy(), 'gt_boxes': b.copy(), 'gt_names': names.copy()})['points']
    exp = restated(proc, np.concatenate([np.zeros((len(kept), 1), f32), kept], 1), [len(kept)])
    nv = int(exp['n_voxels'][0])
    assert same_bits(d['voxels'], exp['voxels'][:nv]) and same_bits(d['voxel_num_points'], exp['voxel_num_points'][:nv])
    assert same_bits(d['voxel_coords'], np.ascontiguousarray(exp['voxel_coords'][:nv, 1:])) and d['voxel_coords'].shape == (nv, 3)
    assert same_bits(d['points'], kept)
    tail = proc.forward({'points': p.copy(), 'gt_boxes': b.copy(), 'gt_names': names.copy(), 'use_lead_xyz': False})
    assert same_bits(np.ascontiguousarray(tail['voxels']), np.ascontiguousarray(exp['voxels'][:nv, :, 3:]))


# ---- end to end: a KITTI directory -> KittiDataset with the hard-voxel processor list -> MeanVFE ---------------------------
from tests import centerpoint_cases as C  # noqa: E402
from tests import ingest_cases as KC  # noqa: E402


def kitti_cfg():
    return {'DATA_SPLIT': {'train': 'train', 'test': 'train'},
            'INFO_PATH': {'train': ['kitti_infos_train.pkl'], 'test': ['kitti_infos_train.pkl']},
            'FOV_POINTS_ONLY': True, 'POINT_CLOUD_RANGE': C.SMALL_DATASET['point_cloud_range'],
            'DATA_PROCESSOR': [{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True},
                               {'NAME': 'shuffle_points', 'SHUFFLE_ENABLED': {'train': False, 'test': False}},
                               {'NAME': 'transform_points_to_voxels', 'VOXEL_SIZE': [0.2, 0.2, 0.5],
                                'MAX_POINTS_PER_VOXEL': 4, 'MAX_NUMBER_OF_VOXELS': {'train': 700, 'test': 900}}]}


@pytest.fixture(scope="module")
def kitti_root(tmp_path_factory):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import create_kitti_infos
    root = str(tmp_path_factory.mktemp("kitti_hvox"))
    KC.write_kitti(root, KC.all_frames(), split='train')
    plain = kitti_cfg()
    plain['DATA_PROCESSOR'] = plain['DATA_PROCESSOR'][:1]
    create_kitti_infos(plain, KC.CLASSES, root, root, workers=2)
    return root


def test_mean_vfe_is_fed_from_a_kitti_directory(kitti_root):
    """The test that shows the feature: before it, DataProcessor refused the entry at construction."""
    import torch
    from dfu3d_amd.pcdet_kitti.kitti_dataset import KittiDataset
    from dfu3d_amd.pcdet_kitti.mean_vfe import MeanVFE
    ds = KittiDataset(kitti_cfg(), KC.CLASSES, training=True, root_path=kitti_root, device=DEV)
    vc = ds.data_processor.voxel_config()
    assert vc['max_voxels'] == 700 and list(ds.grid_size) == vc['grid_size'] and ds.voxel_size == [0.2, 0.2, 0.5]
    vfe = MeanVFE({}, ds.point_feature_encoder.num_point_features)
    seen, capped = 0, False
    for batch in ds.batches(2):
        exp = restated(ds.data_processor, batch['points'].cpu().numpy(), batch['point_cnt'].cpu().numpy())
        nv = int(exp['n_voxels'][0])
        out = vfe(batch)
        assert out['voxel_features'].dtype == torch.float32 and tuple(out['voxel_features'].shape) == (nv, 4)
        assert same_bits(out['voxel_features'].cpu().numpy(), exp['voxel_mean'][:nv])
        assert same_bits(batch['voxel_coords'].cpu().numpy(), exp['voxel_coords'][:nv])
        assert same_bits(batch['voxels'].cpu().numpy(), exp['voxels'][:nv])
        assert same_bits(batch['voxel_num_points'].cpu().numpy(), exp['voxel_num_points'][:nv])
        assert same_bits(batch['voxel_cnt'].cpu().numpy(), exp['voxel_cnt']) and exp['voxel_cnt'].min() > 0
        capped |= bool((exp['point_voxel'][:int(batch['point_cnt'].sum())] < 0).any())
        seen += 1
    assert seen == 3 and capped                                  # some row met a full voxel or the voxel cap
