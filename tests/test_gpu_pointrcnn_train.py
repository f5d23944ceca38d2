"""GPU: PointRCNN(trainable=True) on the small model of golden G20 over a synthetic batch (B = 2, N = 256, boxes placed
around points of the cloud): a training forward and backward, reproducible targets, three iterations of the existing
train_one_epoch, and the way back to a default model for evaluation."""
import numpy as np
import pytest

from tests import optimizer_cases as K
from tests import roipoint_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
B, N, G = 2, 256, 6
TB_KEYS = ['point_loss_box', 'point_loss_cls', 'point_pos_num', 'rcnn_loss', 'rcnn_loss_cls', 'rcnn_loss_corner', 'rcnn_loss_reg']


def batch(seed):
    """points (B * N, 5) [sample, x, y, z, intensity], gt_boxes (B, G, 8): four boxes per sample around points of the
    cloud, each with a cluster of points inside, two rows of padding."""
    import torch
    rng = np.random.default_rng(seed)
    pts = np.zeros((B, N, 4), np.float32)
    pts[..., 0] = rng.uniform(2.0, 30.0, (B, N))
    pts[..., 1] = rng.uniform(-12.0, 12.0, (B, N))
    pts[..., 2] = rng.uniform(-1.5, 0.5, (B, N))
    pts[..., 3] = rng.random((B, N))
    gt = np.zeros((B, G, 8), np.float32)
    sizes = np.array([[3.9, 1.6, 1.56], [0.8, 0.6, 1.73], [1.76, 0.6, 1.73]], np.float32)
    for b in range(B):
        for g in range(G - 2):
            cls = g % 3 + 1
            centre = pts[b, 40 * g, :3].copy()
            gt[b, g] = [*centre, *(sizes[cls - 1] * rng.uniform(0.9, 1.1)), rng.uniform(-np.pi, np.pi), cls]
            k = np.arange(40 * g + 1, 40 * g + 25)
            local = rng.uniform(-0.45, 0.45, (len(k), 3)) * gt[b, g, 3:6]
            c, s = np.cos(gt[b, g, 6]), np.sin(gt[b, g, 6])
            pts[b, k, 0] = centre[0] + local[:, 0] * c - local[:, 1] * s
            pts[b, k, 1] = centre[1] + local[:, 0] * s + local[:, 1] * c
            pts[b, k, 2] = centre[2] + local[:, 2]
    stacked = np.concatenate([np.repeat(np.arange(B), N)[:, None].astype(np.float32), pts.reshape(-1, 4)], axis=1)
    return {'points': torch.from_numpy(stacked).to(DEV), 'gt_boxes': torch.from_numpy(gt).to(DEV), 'batch_size': B}


def model_of(seed, trainable=True):
    import torch
    from dfu3d_amd.pcdet_kitti.point_rcnn import PointRCNN
    torch.manual_seed(seed)
    return PointRCNN(R.g20_model_cfg(), len(R.G20_CLASSES), class_names=R.G20_CLASSES, num_point_features=3 + R.G20_EXTRA,
                     trainable=trainable).to(DEV)


def test_training_forward_and_backward():
    import torch
    model = model_of(3).train()
    gen = torch.Generator(device=DEV)
    model.roi_head.proposal_target_layer.generator = gen
    gen.manual_seed(11)
    ret, tb_dict, disp_dict = model(dict(batch(1)))
    loss = ret['loss']
    assert sorted(tb_dict) == TB_KEYS and all(isinstance(v, float) and np.isfinite(v) for v in tb_dict.values()), tb_dict
    assert loss.dim() == 0 and bool(torch.isfinite(loss)) and disp_dict == {}
    assert tb_dict['point_pos_num'] >= 2 * 4 * 20                      # the clusters inside the boxes are positives
    assert float(loss.detach()) == pytest.approx(tb_dict['point_loss_cls'] + tb_dict['point_loss_box'] + tb_dict['rcnn_loss'], rel=1e-5)
    assert tb_dict['rcnn_loss'] == pytest.approx(tb_dict['rcnn_loss_cls'] + tb_dict['rcnn_loss_reg'] + tb_dict['rcnn_loss_corner'], rel=1e-5)
    first = {k: v.clone() for k, v in model.roi_head.forward_ret_dict.items() if torch.is_tensor(v) and not v.requires_grad}
    labels = model.point_head.forward_ret_dict['point_cls_labels'].clone()
    assert tuple(first['rois'].shape) == (B, 128, 7) and tuple(first['sampled_inds'].shape) == (B, 128)
    assert tuple(labels.shape) == (B * N,) and labels.dtype == torch.int64
    model.roi_head.proposal_target_layer.check_status()
    loss.backward()
    missing = [n for n, p in model.named_parameters() if p.grad is None]
    assert not missing, missing
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters())
    assert any(float(p.grad.abs().max()) > 0 for n, p in model.named_parameters() if n.startswith('backbone_3d'))
    assert float(model.point_head.box_layers[-1].weight.grad.abs().max()) > 0
    assert float(model.roi_head.cls_layers[-1].weight.grad.abs().max()) > 0
    # the same seed again: the same bits of every target
    gen.manual_seed(11)
    model.zero_grad()
    _, tb_again, _ = model(dict(batch(1)))
    again = model.roi_head.forward_ret_dict
    for k, v in first.items():
        assert torch.equal(again[k], v), k
    assert torch.equal(model.point_head.forward_ret_dict['point_cls_labels'], labels)
    # as_tensors: the same numbers without a copy to the host
    loss_t, tb_t, _ = model.get_training_loss(as_tensors=True)
    assert sorted(tb_t) == TB_KEYS and all(torch.is_tensor(v) and v.dim() == 0 and v.is_cuda for v in tb_t.values())
    assert {k: float(v) for k, v in tb_t.items()} == pytest.approx(tb_again, rel=1e-6)


class Loader:
    def __init__(self):
        self.batches = [batch(1), batch(2), batch(1)]

    def __len__(self):
        return len(self.batches)

    def __iter__(self):
        return iter(self.batches)


def test_three_iterations_a_checkpoint_and_the_way_back(tmp_path):
    import torch
    from dfu3d_amd.train_utils import train_utils as T
    from dfu3d_amd.train_utils.optimization import build_optimizer, build_scheduler
    loader = Loader()
    cfg = K.optim_cfg()
    model = model_of(4)
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    opt = build_optimizer(model, cfg)
    sched, _ = build_scheduler(opt, len(loader), 1, -1, cfg)
    rows = []

    class Tb:
        def add_scalar(self, tag, value, step):
            rows.append((tag, float(value), step))
    done = T.train_one_epoch(model, opt, loader, T.model_fn_decorator(), sched, 0, cfg, 0, None, len(loader), iter(loader),
                             tb_log=Tb(), cur_epoch=0, total_epochs=1)
    assert done == 3 and int(model.global_step) == 3
    losses = [v for tag, v, _ in rows if tag == 'train/loss']
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert {tag for tag, _, _ in rows} >= {'train/' + k for k in TB_KEYS}
    after = model.state_dict()
    changed = [k for k in before if k != 'global_step' and not k.endswith('num_batches_tracked') and not torch.equal(before[k], after[k])]
    assert len(changed) >= 0.9 * len([k for k, _ in model.named_parameters()]), len(changed)
    model.roi_head.proposal_target_layer.check_status()
    path = str(tmp_path / 'checkpoint_epoch_1')
    T.save_checkpoint(T.checkpoint_state(model, opt, 1, done), filename=path)
    plain = model_of(9, trainable=False)
    assert not plain.trainable
    ck = plain.load_params_from_file(path + '.pth')                    # strict=True
    assert ck['epoch'] == 1 and all(torch.equal(v, after[k]) for k, v in plain.state_dict().items())
    preds, recall = plain.eval()(dict(batch(2)))
    assert len(preds) == B and all(sorted(p) == ['pred_boxes', 'pred_labels', 'pred_scores'] for p in preds)
    assert all(bool(torch.isfinite(p['pred_boxes']).all()) for p in preds) and recall['gt'] == 2 * (G - 2)
    with pytest.raises(NotImplementedError, match="training row"):
        plain.train()(dict(batch(2)))
