"""GPU: KittiDataset over a temporary KITTI directory of six frames (the three of golden G18, three more): the info
builder against the reference's infos and tests/ingest_ref.py, ds[i] against the reference recipe in NumPy, the batched
form against prepare_batch over the per-frame dicts (and CUDA-tensor points handed to prepare_batch and to
DataBaseSampler.upload_batch directly), two iterations of train_model fed by `batches`, and eval_one_epoch."""
import os
import pickle

import numpy as np
import pytest

from tests import centerpoint_cases as C
from tests import ingest_cases as K
from tests import ingest_ref as R
from tests import optimizer_cases as OC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CLASSES = K.CLASSES
# the small model of tests/centerpoint_cases.py with the class names of these frames
MODEL = dict(C.SMALL_MODEL, DENSE_HEAD=C.dense_head_cfg([['Car'], ['Pedestrian', 'Bicycle']], 8, 4, 20, 50, 20))
DATASET = dict(C.SMALL_DATASET, class_names=CLASSES)


def _cfg(**over):
    ds = C.SMALL_DATASET
    cfg = {'DATA_SPLIT': {'train': 'train', 'test': 'train'},
           'INFO_PATH': {'train': ['kitti_infos_train.pkl'], 'test': ['kitti_infos_train.pkl']},
           'FOV_POINTS_ONLY': True, 'POINT_CLOUD_RANGE': ds['point_cloud_range'],
           'DATA_PROCESSOR': [{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True},
                              {'NAME': 'transform_points_to_voxels_placeholder', 'VOXEL_SIZE': ds['voxel_size']}]}
    cfg.update(over)
    return cfg


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """The directory, its frames and the infos create_kitti_infos wrote (once for the module)."""
    from dfu3d_amd.pcdet_kitti.kitti_dataset import create_kitti_infos
    root = str(tmp_path_factory.mktemp("kitti"))
    frames = K.all_frames()
    K.write_kitti(root, frames, split='train')
    written = create_kitti_infos(_cfg(), CLASSES, root, root, workers=2)
    return root, frames, written


def _dataset(root, training, **over):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import KittiDataset
    return KittiDataset(_cfg(**over), CLASSES, training=training, root_path=root, device=DEV)


def _recipe(frame):
    """The reference's cut of one frame in NumPy."""
    return frame['points'][R.fov_flag(frame['points'], K.calib_of(frame), frame['shape'])]


def test_create_kitti_infos(tree):
    from dfu3d_amd.labels import LabelObject
    from dfu3d_amd.pcdet_kitti.kitti_dataset import annotations_of
    root, frames, written = tree
    assert len(frames) == 6 and all(1400 < len(f["points"]) < 2600 for f in frames)
    assert list(written) == ['kitti_infos_train.pkl']                  # one split named twice: one file, no trainval
    with open(os.path.join(root, 'kitti_infos_train.pkl'), 'rb') as fh:
        infos = pickle.load(fh)
    assert len(infos) == 6
    G = K.golden()
    for i in range(3):                                                 # the reference's own infos
        for k in K.INFO_KEYS:
            got, want = infos[i]['annos'][k], G['f%d_ann_%s' % (i, k)]
            assert got.tolist() == want.tolist() and (k == 'name' or got.dtype == want.dtype), (i, k)
    labelled = []
    for f, info in zip(frames, infos):
        ann = info['annos']
        rows = [l for l in f['label'].splitlines() if l.strip()]
        want = annotations_of([LabelObject(l) for l in rows], K.calib_of(f))
        assert all(np.array_equal(ann[k], want[k]) for k in want)
        boxes = ann['gt_boxes_lidar']
        n_obj = len(boxes)
        labelled.append(n_obj)
        assert n_obj == sum(not l.startswith('DontCare') for l in rows) and ann['num_points_in_gt'].dtype == np.int32
        assert np.array_equal(ann['num_points_in_gt'][:n_obj], R.box_counts(_recipe(f), boxes))
        assert (ann['num_points_in_gt'][n_obj:] == -1).all() and len(ann['num_points_in_gt']) == len(rows)
        assert info['image']['image_shape'].tolist() == f['shape'].tolist()
    assert labelled == [5, 0, 4, 3, 8, 5] and infos[0]['annos']['name'][-1] == 'DontCare'


def test_getitem_equals_the_reference_recipe(tree):
    root, frames, _ = tree
    ds = _dataset(root, True)
    assert len(ds) == 6
    G = K.golden()
    for i, f in enumerate(frames):
        d = ds[i]
        assert sorted(d) == ['calib', 'frame_id', 'gt_boxes', 'gt_names', 'image_shape', 'points']
        want = _recipe(f)
        assert d['points'].dtype == np.float32 and d['points'].shape == want.shape
        assert d['points'].tobytes() == want.tobytes() and 0 < len(want) < len(f['points'])
        assert d['frame_id'] == f['id'] and d['image_shape'].tolist() == f['shape'].tolist()
        assert set(d['gt_names'].tolist()) <= set(CLASSES) and d['gt_boxes'].shape == (len(d['gt_names']), 8)
        assert d['gt_boxes'][:, 7].tolist() == [CLASSES.index(n) + 1 for n in d['gt_names']]
        if i < 3 and len(d['gt_names']):                                # the reference's boxes, its class selection applied
            sel = np.isin(G['f%d_getitem_names' % i], CLASSES)
            assert np.array_equal(d['gt_boxes'][:, :7], G['f%d_getitem_boxes' % i][sel])
    assert len(ds[1]['gt_names']) == 0 and ds[1]['gt_boxes'].shape == (0, 8)
    # FOV_POINTS_ONLY off: the file as it is
    assert _dataset(root, True, FOV_POINTS_ONLY=False)[2]['points'].tobytes() == frames[2]['points'].tobytes()


def _numpy_dicts(ds, idx):
    out = []
    for i in idx:
        d = ds[i]
        out.append({'points': d['points'], 'gt_boxes': d['gt_boxes'][:, :7], 'gt_names': d['gt_names']})
    return out


def test_batches_equal_prepare_batch_over_the_frames(tree, tmp_path):
    import torch
    from dfu3d_amd.pcdet_kitti.data_augmentor import prepare_batch
    from dfu3d_amd.pcdet_kitti.database_sampler import DataBaseSampler
    from tests.gt_sampling_ref import write_database
    root, frames, _ = tree
    ds = _dataset(root, True)
    assert ds.data_augmentor is None                                    # the world augmentor is off
    loader = ds.batches(2)
    assert len(loader) == 3 and loader.dataset is ds
    seen = 0
    for k, batch in enumerate(loader):
        idx = [2 * k, 2 * k + 1]
        dicts = _numpy_dicts(ds, idx)
        want = prepare_batch(dicts, None, ds.data_processor, CLASSES, training=True)
        assert batch['batch_size'] == 2 and batch['points'].is_cuda and batch['points'].shape[1] == 5
        assert torch.equal(batch['points'], want['points']) and torch.equal(batch['gt_boxes'], want['gt_boxes'])
        assert torch.equal(batch['gt_cnt'], want['gt_cnt']) and torch.equal(batch['point_cnt'], want['point_cnt'])
        assert batch['frame_id'] == [frames[i]['id'] for i in idx]
        assert [s.tolist() for s in batch['image_shape']] == [frames[i]['shape'].tolist() for i in idx]
        assert [c.P2.tolist() for c in batch['calib']] == [frames[i]['P2'].tolist() for i in idx]
        seen += batch['points'].shape[0]
        # the same scenes with their points already on the device, handed to prepare_batch directly
        on_dev = [dict(d, points=torch.from_numpy(d['points']).to(DEV)) for d in dicts]
        got = prepare_batch(on_dev, None, ds.data_processor, CLASSES, training=True)
        assert torch.equal(got['points'], want['points']) and torch.equal(got['gt_boxes'], want['gt_boxes'])
        mixed = [on_dev[0], dicts[1]]
        assert torch.equal(prepare_batch(mixed, None, ds.data_processor, CLASSES, training=True)['points'], want['points'])
    assert seen > 1000
    # shuffle and drop_last: a permutation of the frames, the same for the same seed
    order = [b['frame_id'] for b in ds.batches(4, shuffle=True, seed=5, drop_last=True)]
    assert len(order) == 1 and len(order[0]) == 4 and order == [b['frame_id'] for b in ds.batches(4, shuffle=True, seed=5, drop_last=True)]
    assert sorted(f for b in ds.batches(4, shuffle=True, seed=6) for f in b['frame_id']) == [f['id'] for f in frames]
    # through the ground-truth sampler's upload, with a database of two objects
    rng = np.random.default_rng(77)
    db_boxes = np.array([[9.0, 7.0, -1.0, 3.9, 1.6, 1.5, 0.2], [14.0, -8.0, -0.9, 0.8, 0.7, 1.8, 1.0]])
    db_pts = [np.concatenate([rng.uniform(-0.4, 0.4, (30, 3)) * b[3:6], rng.random((30, 1))], 1).astype(np.float32)
              for b in db_boxes]
    write_database(tmp_path, ['Car', 'Pedestrian'], db_boxes, [30, 30], db_pts)
    sampler = DataBaseSampler(tmp_path, {'DB_INFO_PATH': ['kitti_dbinfos_train.pkl'], 'PREPARE': {},
                                         'SAMPLE_GROUPS': ['Car:1', 'Pedestrian:1'], 'NUM_POINT_FEATURES': 4,
                                         'REMOVE_EXTRA_WIDTH': [0.0, 0.0, 0.0], 'LIMIT_WHOLE_SCENE': False}, ['Car', 'Pedestrian'],
                              device=DEV)
    dicts = _numpy_dicts(ds, [0, 4])
    for d in dicts:
        d['gt_boxes_mask'] = np.ones(len(d['gt_boxes']), np.bool_)
    on_dev = [dict(d, points=torch.from_numpy(d['points']).to(DEV)) for d in dicts]
    np.random.seed(11)
    a = sampler.upload_batch([dict(d) for d in dicts])
    np.random.seed(11)
    b = sampler.upload_batch(on_dev)
    assert torch.equal(a['points'], b['points']) and torch.equal(a['pt_off'], b['pt_off']) and a['cap'] == b['cap']
    ga, gb = sampler.launch_batch(a), sampler.launch_batch(b)
    n = int(gb.point_off[-1])                                           # (rows beyond it are capacity, never written)
    assert torch.equal(ga.points[:n], gb.points[:n]) and torch.equal(ga.point_off, gb.point_off) and int(gb.status.item()) == 0
    assert n > 0 and torch.equal(ga.accept, gb.accept) and torch.equal(ga.boxes, gb.boxes)


class Logger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _model(seed):
    import torch
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    torch.manual_seed(seed)
    return CenterPoint(C.cfg(MODEL), len(CLASSES), **DATASET).to(DEV)


def test_train_model_fed_by_batches(tree, tmp_path):
    from dfu3d_amd.train_utils import train_utils as T
    from dfu3d_amd.train_utils.optimization import build_optimizer, build_scheduler
    root, _, _ = tree
    ds = _dataset(root, True)
    loader = ds.batches(3)
    assert len(loader) == 2
    cfg = OC.optim_cfg(PCT_START=0.5)                                   # two steps in all: one up, one down
    model = _model(21)
    assert [int(v) for v in ds.grid_size] == C.SMALL_DATASET['grid_size']
    opt = build_optimizer(model, cfg)
    sched, _ = build_scheduler(opt, len(loader), 1, -1, cfg)
    rows = []

    class Tb:
        def add_scalar(self, tag, value, step):
            rows.append((tag, float(value), step))
    T.train_model(model, opt, loader, T.model_fn_decorator(), sched, cfg, start_epoch=0, total_epochs=1, start_iter=0, rank=0,
                  tb_log=Tb(), ckpt_save_dir=tmp_path, logger=Logger(), logger_iter_interval=1)
    losses = [v for t, v, _ in rows if t == 'train/loss']
    print("losses:", losses)
    assert len(losses) == 2 and np.isfinite(losses).all() and min(losses) > 0
    assert int(model.global_step) == 2 and opt.steps == [2] * len(opt.params)
    assert os.listdir(tmp_path) == ['checkpoint_epoch_1.pth']


def test_eval_one_epoch(tree, tmp_path):
    import torch
    from dfu3d_amd.eval_utils.eval_utils import eval_one_epoch
    from dfu3d_amd.pcdet_kitti.kitti_dataset import generate_prediction_dicts
    root, frames, _ = tree
    ds = _dataset(root, False)
    loader = ds.batches(2)
    model = _model(22)
    # an untrained head scores every cell just under the threshold: lift the heat-map biases so that boxes come out
    with torch.no_grad():
        for head in model.dense_head.heads_list:
            head.hm[-1].bias += 1.0
    logger = Logger()
    cfg = C.cfg({'MODEL': MODEL})
    ret = eval_one_epoch(cfg, C.Cfg(save_to_file=True), model, loader, 3, logger, result_dir=tmp_path / 'eval')
    for t in ('0.3', '0.5', '0.7'):
        assert 0.0 <= ret['recall/roi_' + t] <= 1.0 and 0.0 <= ret['recall/rcnn_' + t] <= 1.0
    ap = {k: v for k, v in ret.items() if not k.startswith('recall/')}
    print("AP dictionary:", ap)
    assert ap and all(k.split('_')[0] in CLASSES for k in ap) and all(np.isfinite(v) for v in ap.values())
    with open(tmp_path / 'eval' / 'result.pkl', 'rb') as fh:
        annos = pickle.load(fh)
    assert [a['frame_id'] for a in annos] == [f['id'] for f in frames]
    assert sorted(os.listdir(tmp_path / 'eval' / 'final_result' / 'data')) == [f['id'] + '.txt' for f in frames]
    assert sum(len(a['name']) for a in annos) > 0
    for a in annos:
        with open(tmp_path / 'eval' / 'final_result' / 'data' / (a['frame_id'] + '.txt')) as fh:
            assert len(fh.readlines()) == len(a['name'])
    assert any('recall_rcnn_0.3' in l for l in logger.lines) and any('EPOCH 3 EVALUATION' in l for l in logger.lines)
    assert not model.training
    # by hand on the same batches
    by_hand = []
    with torch.no_grad():
        for batch in ds.batches(2):
            assert 'gt_boxes' in batch                                  # the infos have annotations: the recall record
            pred, _ = model(batch)
            by_hand += generate_prediction_dicts(batch, pred, CLASSES)
    assert len(by_hand) == len(annos) == 6
    for a, b in zip(annos, by_hand):
        assert sorted(a) == sorted(b)
        for k in a:
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (a['frame_id'], k)
