"""GPU: train_model of dfu3d_amd/train_utils on the small CenterPoint (tests/centerpoint_cases.py SMALL_MODEL) over a
loader of two batches that repeat: 2 epochs x 10 iterations with the fused one-cycle optimiser, the checkpoints, and a
resume from the first of them.  Whole-model parameters are not compared bit for bit across runs: the convolution
algorithm is the vendor library's choice."""
import os

import numpy as np
import pytest

from tests import centerpoint_cases as C
from tests import optimizer_cases as K

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ITERS, EPOCHS = 10, 2


def _scenes(seed, boxes):
    """Two scenes: a few thousand points, dense inside every box."""
    rng = np.random.default_rng(seed)
    r = C.SMALL_DATASET['point_cloud_range']
    out = []
    for s, rows in enumerate(boxes):
        n = 2500 + 700 * s
        pts = np.stack([rng.uniform(r[0] - 2, r[3] + 2, n), rng.uniform(r[1] - 2, r[4] + 2, n), rng.uniform(-2.5, 0.5, n),
                        rng.random(n)], 1)
        for b in rows:
            k = 60
            inside = np.stack([b[0] + rng.uniform(-0.5, 0.5, k) * b[3], b[1] + rng.uniform(-0.5, 0.5, k) * b[4],
                               b[2] + rng.uniform(-0.5, 0.5, k) * b[5], rng.random(k)], 1)
            pts = np.concatenate([pts, inside], 0)
        out.append({'points': pts.astype(np.float32), 'gt_boxes': np.array([b[:7] for b in rows], np.float32),
                    'gt_names': np.array([b[7] for b in rows])})
    return out


BOXES = [
    [[[8.0, -4.0, -1.0, 3.9, 1.6, 1.5, 0.3, 'Car'], [20.0, 5.0, -1.0, 4.2, 1.8, 1.6, -1.2, 'Car'],
      [12.0, 2.0, -0.8, 0.7, 0.7, 1.7, 0.0, 'Pedestrian']],
     [[15.0, -6.0, -1.0, 1.8, 0.6, 1.6, 2.0, 'Cyclist'], [25.0, 8.0, -0.9, 0.8, 0.8, 1.8, 0.5, 'Pedestrian'],
      [5.0, 0.0, -1.0, 4.1, 1.7, 1.5, 3.0, 'Car']]],
    [[[10.0, 3.0, -1.0, 4.0, 1.7, 1.5, 1.0, 'Car'], [22.0, -7.0, -0.9, 0.8, 0.7, 1.8, 0.2, 'Pedestrian'],
      [27.0, 4.0, -1.0, 1.7, 0.6, 1.6, -0.7, 'Cyclist']],
     [[6.0, -8.0, -1.0, 3.8, 1.6, 1.4, 2.5, 'Car'], [18.0, 0.0, -1.0, 4.3, 1.8, 1.6, 0.1, 'Car'],
      [13.0, 9.0, -0.8, 0.7, 0.7, 1.7, 1.4, 'Pedestrian']]],
]


class Loader:
    """Two batches that repeat, ITERS per epoch; every epoch begins and ends with b0, b1, b0."""

    def __init__(self):
        from dfu3d_amd.pcdet_kitti.data_augmentor import prepare_batch
        from dfu3d_amd.pcdet_kitti.data_processor import DataProcessor
        ds = C.SMALL_DATASET
        proc = DataProcessor([C.Cfg(NAME='mask_points_and_boxes_outside_range', REMOVE_OUTSIDE_BOXES=True),
                              C.Cfg(NAME='transform_points_to_voxels_placeholder', VOXEL_SIZE=ds['voxel_size'])],
                             np.array(ds['point_cloud_range'], np.float32), True, 4, device=DEV)
        b = [prepare_batch(_scenes(1700 + k, BOXES[k]), None, proc, ds['class_names'], training=True) for k in (0, 1)]
        self.keys = [sorted(x) for x in b]
        self.order = [b[k] for k in (0, 1, 0, 1, 0, 1, 0, 0, 1, 0)]

    def __len__(self):
        return len(self.order)

    def __iter__(self):
        return iter(self.order)


class TbLog:
    def __init__(self):
        self.rows = []

    def add_scalar(self, tag, value, step):
        self.rows.append((tag, value, step))

    def of(self, tag):
        return [(v, s) for t, v, s in self.rows if t == tag]


class Logger:
    def __init__(self):
        self.lines = []

    def info(self, msg):
        self.lines.append(msg)


def _model(seed):
    import torch
    from dfu3d_amd.pcdet_kitti.centerpoint import CenterPoint
    torch.manual_seed(seed)
    return CenterPoint(C.cfg(C.SMALL_MODEL), len(C.SMALL_CLASSES), **C.SMALL_DATASET).to(DEV)


def _schedule_lrs():
    from dfu3d_amd.train_utils.optimization.learning_schedules_fastai import OneCycle

    class H:
        lr = mom = 0
    h = H()
    s = OneCycle(h, ITERS * EPOCHS, K.LR, list(K.OPTIMIZATION['MOMS']), K.OPTIMIZATION['DIV_FACTOR'], K.OPTIMIZATION['PCT_START'])
    out = []
    for i in range(ITERS * EPOCHS):
        s.step(i)
        out.append(float(h.lr))
    return out


def _setup(seed, loader):
    from dfu3d_amd.train_utils.optimization import build_optimizer, build_scheduler
    cfg = K.optim_cfg()
    model = _model(seed)
    opt = build_optimizer(model, cfg)
    sched, warm = build_scheduler(opt, len(loader), EPOCHS, -1, cfg)
    assert warm is None
    return cfg, model, opt, sched


def test_train_model_and_resume(tmp_path):
    import torch
    from dfu3d_amd.train_utils import train_utils as T
    loader = Loader()
    assert len(loader) == ITERS
    cfg, model, opt, sched = _setup(17, loader)
    n_tensors = len(opt.params)
    tb, logger = TbLog(), Logger()
    T.train_model(model, opt, loader, T.model_fn_decorator(), sched, cfg, start_epoch=0, total_epochs=EPOCHS, start_iter=0,
                  rank=0, tb_log=tb, ckpt_save_dir=tmp_path, logger=logger, logger_iter_interval=5)
    assert [sorted(b) for b in loader.order[:2]] == loader.keys          # the loader's dicts are as they were made
    losses = [float(v) for v, _ in tb.of('train/loss')]
    print("losses:", " ".join("%.4f" % x for x in losses))
    assert len(losses) == ITERS * EPOCHS and np.isfinite(losses).all()
    assert [s for _, s in tb.of('train/loss')] == list(range(1, ITERS * EPOCHS + 1))
    assert np.mean(losses[-3:]) < np.mean(losses[:3]), losses
    # the loss of tb_dict is the one the step was taken on
    assert [v for v, _ in tb.of('train/loss_rpn')] == pytest.approx(losses, rel=1e-6)
    want = _schedule_lrs()
    lrs = tb.of('meta_data/learning_rate')
    assert len(lrs) == 2 * ITERS * EPOCHS
    assert [v for v, _ in lrs[0::2]] == want and [s for _, s in lrs[0::2]] == list(range(ITERS * EPOCHS))
    assert [v for v, _ in lrs[1::2]] == want
    assert int(model.global_step) == ITERS * EPOCHS and opt.steps == [ITERS * EPOCHS] * n_tensors
    # the norm and the status are read at the logging interval, the first and the last iteration of an epoch
    assert [s for _, s in tb.of('train/grad_norm')] == [1, 5, 10, 11, 15, 20]
    assert all(np.isfinite(v) and v > 0 for v, _ in tb.of('train/grad_norm')) and len(logger.lines) == 6
    for e in (1, 2):
        ck = torch.load(str(tmp_path / ('checkpoint_epoch_%d.pth' % e)), map_location='cpu')
        assert sorted(ck) == ['epoch', 'it', 'model_state', 'optimizer_state', 'version']
        assert (ck['epoch'], ck['it']) == (e, e * ITERS) and list(ck['model_state']) == list(model.state_dict())
        assert sorted(ck['optimizer_state']) == ['param_groups', 'state'] and len(ck['optimizer_state']['state']) == n_tensors
    assert sorted(os.listdir(tmp_path)) == ['checkpoint_epoch_1.pth', 'checkpoint_epoch_2.pth']

    # a fresh model and optimiser resume from epoch 1
    cfg, model2, opt2, sched2 = _setup(18, loader)
    ck = model2.load_params_from_file(str(tmp_path / 'checkpoint_epoch_1.pth'))      # strict=True
    opt2.load_state_dict(ck['optimizer_state'])
    assert (ck['epoch'], ck['it']) == (1, ITERS) and opt2.steps == [ITERS] * n_tensors and int(model2.global_step) == ITERS
    tb2 = TbLog()
    T.train_model(model2, opt2, loader, T.model_fn_decorator(), sched2, cfg, start_epoch=ck['epoch'], total_epochs=EPOCHS,
                  start_iter=ck['it'], rank=0, tb_log=tb2, ckpt_save_dir=tmp_path, max_ckpt_save_num=2)
    lrs2 = tb2.of('meta_data/learning_rate')
    assert lrs2[0] == (want[ITERS], ITERS) and [v for v, _ in lrs2[0::2]] == want[ITERS:]
    assert int(model2.global_step) == ITERS * EPOCHS and opt2.steps == [ITERS * EPOCHS] * n_tensors
    losses2 = [float(v) for v, _ in tb2.of('train/loss')]
    print("resumed losses:", " ".join("%.4f" % x for x in losses2))
    assert len(losses2) == ITERS and np.isfinite(losses2).all()
    # the same state and the same batch: the first resumed loss is one forward pass away from the first run's (float32
    # sums in another order at most: some 1e-6 relative per layer; not bit for bit, the convolutions are the vendor's)
    assert losses2[0] == pytest.approx(losses[ITERS], rel=1e-3)
    # rotation: at most max_ckpt_save_num files, the oldest removed first
    assert sorted(os.listdir(tmp_path)) == ['checkpoint_epoch_2.pth']
