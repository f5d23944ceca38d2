"""GPU: the world-augmentation stage (worldaug_stage.hip, include/dfu3d_aug.h) and its Python surface against the NumPy
restatement (bit for bit) and golden G15 (as tests/test_oracle_world_aug.py compares the restatement with it)."""
import ctypes
import json

import numpy as np
import pytest

from tests import world_aug_cases as W
from tests import world_aug_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


class Cfg(dict):
    __getattr__ = dict.__getitem__


def _operands(ops):
    import torch
    from dfu3d_amd import stages as st
    from dfu3d_amd.pcdet_kitti.data_augmentor import params_record
    pts = np.concatenate([o[0] for o in ops], 0)
    boxes = np.concatenate([o[1] for o in ops], 0)
    npts = np.array([len(o[0]) for o in ops], np.int64)
    nbox = np.array([len(o[1]) for o in ops], np.int64)

    def h2d(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return (h2d(pts), h2d(np.r_[0, np.cumsum(npts)].astype(np.int64)), h2d(boxes),
            h2d(np.r_[0, np.cumsum(nbox)].astype(np.int32)), h2d(nbox.astype(np.int32)),
            h2d(np.concatenate([o[2] for o in ops], 0).astype(np.int32)),
            h2d(st.aug_params([params_record(o[3]) for o in ops]))), int(max(nbox.max(), 1))


def _run(ops, pc_range, mask_boxes=True, **kw):
    import torch
    from dfu3d_amd import stages as st
    args, cap = _operands(ops)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    mode = st.AUG_MASK_POINTS | st.AUG_FILTER_CLASS | (st.AUG_MASK_BOXES if mask_boxes else 0)
    out = st.world_aug_collate(*args, torch.from_numpy(np.asarray(pc_range, np.float32)).to(DEV), mode, cap, status, **kw)
    return [None if t is None else t.cpu().numpy() for t in out], int(status.item())


def _ops(ci, scenes):
    out = []
    for s in scenes:
        p, b, names = W.inputs(ci, s)
        out.append((p, b, R.class_ids(names, W.class_names()), W.drawn(ci, s)))
    return out


def _check_against_restatement(got, want, n_rows):
    (out, n_kept, point_cnt, gt, gt_cnt, _, _), status = got
    pts, wgt, wpc, wgc = want
    assert status == 0
    assert int(n_kept[0]) == len(pts) and np.array_equal(point_cnt, wpc) and np.array_equal(gt_cnt, wgc)
    assert W.same_bits(out[:len(pts)], pts)
    tail = out[len(pts):]
    assert len(out) == n_rows and np.all(tail[:, 0] == -1) and not tail[:, 1:].any()      # the padded tail is defined
    assert W.same_bits(gt[:, :wgt.shape[1]], wgt)
    assert not gt[:, wgt.shape[1]:].any()
    for b, k in enumerate(wgc):
        assert not W.bits(gt[b, k:]).any()                                                 # +0, every slot written


@pytest.mark.parametrize("ci", range(W.N_CFG))
def test_every_scene_alone_equals_the_restatement(ci):
    for s in range(W.n_scenes()):
        ops = _ops(ci, [s])
        want = R.batch(ops, W.pc_range(ci), mask_boxes=W.training(ci))
        _check_against_restatement(_run(ops, W.pc_range(ci), W.training(ci)), want, len(ops[0][0]))


@pytest.mark.parametrize("ci", range(W.N_CFG))
def test_one_batch_of_all_scenes_equals_the_restatement_and_the_golden(ci):
    """Scene sizes 0, 1, 63, 64, 1023, 1024, 1025, 3000 and the planted ones in one CSR: chunks of 1024 rows straddle
    up to five scenes, and scene 0 is empty."""
    G = W.golden()
    ops = _ops(ci, range(W.n_scenes()))
    got = _run(ops, W.pc_range(ci), W.training(ci))
    _check_against_restatement(got, W.restated(ci)[1], sum(len(o[0]) for o in ops))
    (out, n_kept, _, gt, gt_cnt, _, _), _ = got
    # against the reference's own batch, as the CPU test compares the restatement with it
    assert np.array_equal(out[:int(n_kept[0]), 0].astype(np.int8), G['batch/%d/batch_index' % ci])
    want = G['batch/%d/gt_boxes' % ci]
    assert np.array_equal(gt[:, :want.shape[1], -1], want[:, :, -1])
    big = [s for s in range(W.n_scenes()) if len(W.inputs(ci, s)[1]) >= 64]
    assert W.same_bits(gt[big][:, :want.shape[1]], want[big])
    off = np.r_[0, np.cumsum([int((G['batch/%d/batch_index' % ci] == s).sum()) for s in range(W.n_scenes())])]
    for s in range(W.n_scenes()):
        p = W.inputs(ci, s)[0]
        keep = G['final/%d/%d/point_keep' % (ci, s)]
        assert off[s + 1] - off[s] == keep.sum()                                           # the reference's decisions
        if len(p) >= 64 or W.planted(ci, s):
            assert W.same_bits(out[off[s]:off[s + 1], 1:4], G['aug/%d/%d/xyz' % (ci, s)][keep])
    # two empty scenes side by side inside one chunk and an empty last scene (scene 0 is the empty one)
    ops = _ops(ci, [2, 0, 0, 3, 8, 0])
    want = R.batch(ops, W.pc_range(ci), mask_boxes=W.training(ci))
    assert len(want[0]) > 0
    _check_against_restatement(_run(ops, W.pc_range(ci), W.training(ci)), want, sum(len(o[0]) for o in ops))


def test_rows_beyond_the_last_offset_are_never_read():
    """The point array may be a capacity (the sampler's output is): 1500 rows behind point_off[B], all of them inside
    the range and one NaN, change nothing but the length of the padded tail."""
    import torch
    from dfu3d_amd import stages as st
    ops = _ops(0, [4, 1, 6])
    want = R.batch(ops, W.pc_range(0))
    args, cap = _operands(ops)
    extra = torch.full((1500, 4), 10.0, device=DEV)
    extra[7, 0] = float('nan')
    args = (torch.cat([args[0], extra]).contiguous(),) + args[1:]
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = st.world_aug_collate(*args, torch.from_numpy(W.pc_range(0)).to(DEV),
                               st.AUG_MASK_POINTS | st.AUG_FILTER_CLASS | st.AUG_MASK_BOXES, cap, status)
    got = [None if t is None else t.cpu().numpy() for t in out], int(status.item())
    _check_against_restatement(got, want, sum(len(o[0]) for o in ops) + 1500)


def test_two_runs_give_the_same_bits():
    ops = _ops(0, range(W.n_scenes()))
    a, b = _run(ops, W.pc_range(0)), _run(ops, W.pc_range(0))
    for x, y in zip(a[0], b[0]):
        assert (x is None and y is None) or x.tobytes() == y.tobytes()


def test_transformed_boxes_and_keep_flags():
    """boxes_aug keeps the input's type and rows; box_keep names the rows of gt_boxes."""
    for ci in range(W.N_CFG):
        ops = _ops(ci, [5])
        (_, _, _, gt, gt_cnt, aug, keep), _ = _run(ops, W.pc_range(ci), W.training(ci), want_aug=True, want_keep=True)
        _, fg, wkeep, _, ab, _ = W.restated(ci)[0][5]
        assert W.same_bits(aug, ab) and np.array_equal(keep != 0, wkeep) and int(gt_cnt[0]) == wkeep.sum()


def test_nonfinite_points_and_box_cap_set_status_bits():
    from dfu3d_amd import stages as st
    p = np.zeros((5, 4), np.float32)
    p[1, 0], p[3, 1] = np.nan, np.inf
    b = np.tile(np.array([[1.0, 1.0, 0.0, 1, 1, 1, 0]], np.float32), (3, 1))
    ops = [(p, b, np.ones(3, np.int32), {'flips': []})]
    (out, n_kept, _, gt, gt_cnt, _, _), status = _run(ops, [-5, -5, -5, 5, 5, 5])
    assert status == st.AUG_ST_NONFINITE and int(n_kept[0]) == 3 and int(gt_cnt[0]) == 3
    import torch
    args, _ = _operands(ops)
    word = torch.zeros(1, dtype=torch.int32, device=DEV)
    res = st.world_aug_collate(*args, torch.tensor([-5, -5, -5, 5, 5, 5.0], device=DEV), st.AUG_MASK_BOXES, 2, word)
    assert int(word.item()) == st.AUG_ST_BOX_CAP and int(res[4][0]) == 2 and res[3].shape == (1, 2, 8)


def test_launch_count_does_not_depend_on_the_batch(monkeypatch):
    import torch
    from dfu3d_amd import _lib, _lib_aug
    L = _lib.load_variant("count")
    L.dfu3d_debug_launch_count.restype = ctypes.c_longlong
    L.dfu3d_debug_launch_count.argtypes = [ctypes.c_int]
    monkeypatch.setattr(_lib, "_LIB", L)
    monkeypatch.setattr(_lib_aug, "_BOUND", _lib_aug.bind(L))
    counts = []
    for B in (1, 64):
        ops = [_ops(0, [4 + b % 3])[0] for b in range(B)]
        L.dfu3d_debug_launch_count(1)
        _, status = _run(ops, W.pc_range(0))
        counts.append(int(L.dfu3d_debug_launch_count(1)))
        assert status == 0
    torch.cuda.synchronize()
    assert counts[0] == counts[1] and 0 < counts[0] <= 4, counts


def _surface(ci, planted, device=DEV):
    from dfu3d_amd.pcdet_kitti.data_augmentor import DataAugmentor
    from dfu3d_amd.pcdet_kitti.data_processor import DataProcessor
    cfg = W.dataset_cfg(ci, planted)
    aug = DataAugmentor('.', Cfg(cfg['DATA_AUGMENTOR']), W.class_names(), device=device)
    proc = DataProcessor([Cfg(c) for c in cfg['DATA_PROCESSOR']], W.pc_range(ci), W.training(ci), 4, device=device)
    return aug, proc


@pytest.mark.parametrize("ci", range(W.N_CFG))
def test_forward_per_scene_equals_the_golden_dicts(ci):
    """DataAugmentor.forward, the class filter, DataProcessor.forward at B = 1 under the golden's seed: keys, decisions,
    dtypes; floats bit for bit from 64 rows on (smaller lists: tests/test_oracle_world_aug.py's bound, via the stage ==
    restatement tests above)."""
    from dfu3d_amd.pcdet_kitti.data_augmentor import select_classes
    G = W.golden()
    sets = {pl: _surface(ci, pl) for pl in (False, True)}
    np.random.seed({0: 151, 1: 152}[ci])
    for s in range(W.n_scenes()):
        aug, proc = sets[W.planted(ci, s)]
        p, b, names = W.inputs(ci, s)
        mask = np.array([n in W.class_names() for n in names], dtype=np.bool_)
        d = aug.forward({'points': p.copy(), 'gt_boxes': b.copy(), 'gt_names': names.copy(), 'gt_boxes_mask': mask})
        assert sorted(d.keys()) == list(G['aug/%d/%d/keys' % (ci, s)])
        assert d['noise_rot'] == float(G['drawn/%d/%d/noise_rot' % (ci, s)])
        _, _, _, ap, ab, _ = W.restated(ci)[0][s]
        assert W.same_bits(d['points'], ap) and W.same_bits(d['gt_boxes'], ab[mask])
        assert np.array_equal(d['gt_names'], G['aug/%d/%d/gt_names' % (ci, s)])
        d = proc.forward(select_classes(d, W.class_names()))
        d.pop('gt_names')
        d['lidar_aug_matrix'] = d['use_lead_xyz'] = None      # dataset.py's own keys, not this row's
        assert sorted(d.keys()) == list(G['final/%d/%d/keys' % (ci, s)])
        fp, fg, _, _, _, _ = W.restated(ci)[0][s]
        want = G['final/%d/%d/gt_boxes' % (ci, s)]
        assert W.same_bits(d['points'], fp) and W.same_bits(d['gt_boxes'], fg)
        assert d['gt_boxes'].dtype == want.dtype and W.same_bits(d['gt_boxes'][:, -1], want[:, -1])
        if len(b) >= 64:
            assert W.same_bits(d['gt_boxes'], want)
    st = np.random.get_state()
    assert np.array_equal(st[1], G['rng/%d/keys' % ci]) and st[2] == int(G['rng/%d/pos' % ci])


def _raw_dicts(ci, scenes):
    out = []
    for s in scenes:
        p, b, names = W.inputs(ci, s)
        out.append({'points': p.copy(), 'gt_boxes': b.copy(), 'gt_names': names.copy()})
    return out


def test_prepare_batch_sync_counts_and_nine_column_boxes():
    """The padded form synchronises nowhere, the default form exactly once (torch's sync debug mode counts torch's own
    synchronising calls; the library never synchronises).  Configuration 1: float64 boxes of 9 columns, which only
    scenes that did not come from the sampler can have."""
    import torch
    import warnings
    from dfu3d_amd.pcdet_kitti.data_augmentor import params_record, prepare_batch
    ci = 1
    aug, proc = _surface(ci, False)
    scenes = [3, 4, 0, 7]
    np.random.seed(5)
    pad = prepare_batch(_raw_dicts(ci, scenes), aug, proc, W.class_names(), training=True, as_padded=True)   # warm
    torch.cuda.synchronize()
    np.random.seed(5)
    torch.cuda.set_sync_debug_mode("error")
    try:
        pad = prepare_batch(_raw_dicts(ci, scenes), aug, proc, W.class_names(), training=True, as_padded=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    np.random.seed(5)
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            cut = prepare_batch(_raw_dicts(ci, scenes), aug, proc, W.class_names(), training=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len([x for x in w if "synchroniz" in str(x.message)]) == 1, [str(x.message) for x in w]
    # what it computes: the restatement under the same draws
    np.random.seed(5)
    ops = []
    for s in scenes:
        p, b, names = W.inputs(ci, s)
        ops.append((p, b, R.class_ids(names, W.class_names()), aug.draw_world_params(9)))
    pts, gt, wpc, wgc = R.batch(ops, W.pc_range(ci), mask_boxes=False)        # training=False processor: boxes stay
    assert cut['batch_size'] == 4 and W.same_bits(cut['points'].cpu().numpy(), pts)
    assert W.same_bits(cut['gt_boxes'].cpu().numpy(), gt) and gt.shape[2] == 10
    assert np.array_equal(cut['gt_cnt'].cpu().numpy(), wgc) and cut['empty_scenes'] == [2]
    n = int(pad['n_kept'].item())
    assert n == len(pts) and W.same_bits(pad['points'].cpu().numpy()[:n], pts)
    assert np.all(pad['points'].cpu().numpy()[n:, 0] == -1)


def test_end_to_end_from_the_database_to_the_encoder_and_the_targets(tmp_path):
    """prepare_batch on G11's database and scenes: gt sampling -> augmentation -> masks -> collate on the device; its
    `points` through DynamicPillarVFE and its `gt_boxes` through CenterHead.assign_targets as they are, against the same
    two modules on the restatement's arrays uploaded from the host."""
    import torch
    from dfu3d_amd.pcdet_kitti.data_augmentor import DataAugmentor, prepare_batch
    from dfu3d_amd.pcdet_kitti.data_processor import DataProcessor
    from tests.gt_sampling_ref import write_database
    from tests import test_gpu_center_head as th
    with np.load(W.PATH.replace("g15_world_aug", "g11_gt_sampling")) as z:
        G11 = {k: z[k] for k in z.files}
    classes = [str(c) for c in G11['class_names']]
    off = G11['db_off']
    pts = [G11['db_points'][off[k]:off[k + 1]] for k in range(len(off) - 1)]
    write_database(str(tmp_path), [str(c) for c in G11['db_classes']], G11['db_boxes'], np.diff(off), pts,
                   G11['db_difficulty'])
    world = W.dataset_cfg(0, False)['DATA_AUGMENTOR']['AUG_CONFIG_LIST']
    sampler_cfg = dict(json.loads(str(G11['cfg/0'])), NAME='gt_sampling')
    pc_range = np.array([-25.0, -25.0, -3.0, 25.0, 25.0, 1.0], np.float32)       # inside the scenes' +-32 m: points drop
    proc_cfg = [Cfg(c) for c in W.dataset_cfg(0, False)['DATA_PROCESSOR']]

    def scenes():
        out = []
        for s in range(int(G11['n_scenes'])):
            pre = 'scene/%d/' % s
            out.append({'points': G11[pre + 'points'].copy(), 'gt_boxes': G11[pre + 'gt_boxes'].astype(np.float32),
                        'gt_names': G11[pre + 'gt_names'].copy(), 'gt_boxes_mask': G11[pre + 'mask'].copy()})
        return out
    aug = DataAugmentor(tmp_path, Cfg(AUG_CONFIG_LIST=[Cfg(sampler_cfg)] + [Cfg(c) for c in world], DISABLE_AUG_LIST=[]),
                        classes, device=DEV)
    proc = DataProcessor(proc_cfg, pc_range, True, 4, device=DEV)
    np.random.seed(77)
    batch = prepare_batch(scenes(), aug, proc, classes, training=True)
    # the same on the host: a second sampler state, the sampler's split(), then the restatement under the same draws
    aug2 = DataAugmentor(tmp_path, Cfg(AUG_CONFIG_LIST=[Cfg(sampler_cfg)] + [Cfg(c) for c in world], DISABLE_AUG_LIST=[]),
                         classes, device=DEV)
    np.random.seed(77)
    dicts = aug2.sampler.sample_batch(scenes()).split()
    ops = [(d['points'], d['gt_boxes'], R.class_ids(d['gt_names'], classes), aug2.draw_world_params(7)) for d in dicts]
    wpts, wgt, _, wgc = R.batch(ops, pc_range, mask_boxes=True)
    assert W.same_bits(batch['points'].cpu().numpy(), wpts)
    assert W.same_bits(batch['gt_boxes'].cpu().numpy(), wgt) and np.array_equal(batch['gt_cnt'].cpu().numpy(), wgc)
    assert 0.05 < len(wpts) / sum(len(d['points']) for d in dicts) < 0.95 and wgc.sum() > 0

    from dfu3d_amd.pcdet_kitti.dynamic_pillar_vfe import DynamicPillarVFE
    torch.manual_seed(0)
    vfe = DynamicPillarVFE(model_cfg=dict(USE_NORM=True, WITH_DISTANCE=False, USE_ABSLOTE_XYZ=True, NUM_FILTERS=[32]),
                           num_point_features=4, voxel_size=[0.5, 0.5, 4.0], grid_size=[100, 100, 1],
                           point_cloud_range=[float(v) for v in pc_range]).to(DEV).eval()
    head = th.make_head(dict(class_names=classes, heads=[['Car'], ['Pedestrian', 'Cyclist']],
                             point_cloud_range=[float(v) for v in pc_range], voxel_size=[0.5, 0.5, 4.0], stride=2,
                             num_max_objs=50, gaussian_overlap=0.1, min_radius=2, C=8))
    host = {'batch_size': batch['batch_size'], 'points': torch.from_numpy(wpts).to(DEV),
            'gt_boxes': torch.from_numpy(wgt).to(DEV)}
    with torch.no_grad():
        a, b = vfe({'batch_size': batch['batch_size'], 'points': batch['points']}), vfe(dict(host))
    assert a['pillar_features'].shape[0] > 0
    for key in ('pillar_features', 'voxel_coords'):
        assert a[key].cpu().numpy().tobytes() == b[key].cpu().numpy().tobytes(), key
    ta = th.to_np(head.assign_targets(batch['gt_boxes'], feature_map_size=[50, 50], check=True))
    tb = th.to_np(head.assign_targets(host['gt_boxes'], feature_map_size=[50, 50], check=True))
    assert sorted(ta) == sorted(tb) and sum(float(h.sum()) for h in ta['heatmaps']) > 0
    for key in ta:
        for x, y in zip(ta[key], tb[key]):
            assert x.tobytes() == y.tobytes(), key


def test_more_chunks_than_one_pass_of_the_offset_scan():
    """Just over 1024 x 1024 rows of 4 columns in three scenes, the range mask on: 1025 chunks of 1024 rows, each with
    its own kept count, so the one workgroup that scans the chunk counts 1024 at a time carries its running total
    into a second pass (the last chunk's offset, and n_kept)."""
    rng = np.random.default_rng(41)
    sizes = [400000, 300000, 1024 * 1024 + 700 - 700000]
    assert (sum(sizes) + 1023) // 1024 > 1024                                              # what the test is for
    box = np.array([[1.0, 2.0, -1.0, 4.0, 2.0, 1.5, 0.3]], np.float32)
    ops = []
    for b, n in enumerate(sizes):
        p = np.empty((n, 4), np.float32)
        p[:, :2] = rng.uniform(-50, 50, (n, 2))
        p[:, 2] = rng.uniform(-3, 1, n)
        p[:, 3] = rng.random(n)
        drawn = {'flips': [('x', b == 1), ('y', b == 2)], 'noise_rot': 0.3 - 0.25 * b, 'noise_scale': 0.95 + 0.05 * b,
                 'noise_translate': np.array([[0.5, -0.25, 0.1]], np.float32) * b}
        ops.append((p, box, np.ones(1, np.int32), drawn))
    pc_range = np.array([-40.0, -40.0, -3.0, 40.0, 40.0, 1.0], np.float32)
    want = R.batch(ops, pc_range)
    assert 0.5 < len(want[0]) / sum(sizes) < 0.8 and want[2][-1] > 1024                    # rows drop everywhere
    _check_against_restatement(_run(ops, pc_range), want, sum(sizes))
