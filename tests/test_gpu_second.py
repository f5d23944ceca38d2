"""GPU: the anchor head and the SECOND detector.

The head's three losses, their per-element terms, their gradients and its decoded boxes on golden G25's own predictions
and targets (tests/golden/capture_anchor_head_golden.py: the reference's head on the CPU), every float within
d_hip <= max(4 * d_torch, 4 ulp at the golden's largest magnitude), d_torch being the deviation of a plain formulation in
torch primitives on the same GPU (no code of the head or of its loss classes) -- the rule of goldens G20 and G21.

A small SECONDNet over a KITTI directory (the grid of tests/test_gpu_voxel_centerpoint.py: 128 x 96 x 40 cells, a
feature map of 16 x 12, 1 152 anchors) takes a training step with a finite loss and non-zero gradients in the three
convolutions of the head, trains through train_model and its OptimWrapper, reloads its own checkpoint with strict=True,
returns pred_dicts in evaluation and runs an evaluation epoch."""
import math
import os

import numpy as np
import pytest

from tests import anchor_target_ref as R
from tests import ingest_cases as KC
from tests.centerpoint_cases import Cfg, cfg
from tests.test_gpu_voxel_centerpoint import kitti_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g25_anchor_head.npz")


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _within(name, hip, plain, gold):
    hip, plain = hip.detach().cpu().numpy().reshape(gold.shape), plain.detach().cpu().numpy().reshape(gold.shape)
    d_hip, d_torch = float(np.abs(hip - gold).max()), float(np.abs(plain - gold).max())
    floor = 4.0 * float(np.spacing(np.float32(np.abs(gold).max())))
    print("G25 %-22s d_hip %.3g  d_torch %.3g  floor %.3g  (largest |golden| %.3g)" % (name, d_hip, d_torch, floor, np.abs(gold).max()))
    assert d_hip <= max(4.0 * d_torch, floor), (name, d_hip, d_torch, floor)


# ---- the plain formulation ---------------------------------------------------------------------------------------------------
def plain_losses(g, preds):
    """AnchorHeadTemplate's three losses in torch primitives -> (per-element terms, the four scalars)."""
    import torch
    w = R.HEAD_CFG['LOSS_CONFIG']['LOSS_WEIGHTS']
    labels, targets, anchors = cu(g['box_cls_labels']), cu(g['box_reg_targets']), cu(g['anchors'])
    B = labels.shape[0]
    pos = labels > 0
    norm = pos.sum(1, keepdim=True).float().clamp(min=1.0)
    # classification: sigmoid focal loss over the one-hot of the cared labels, background column dropped
    x = preds['cls_preds'].view(B, -1, 3)
    t = torch.nn.functional.one_hot((labels * (labels >= 0)).long(), 4)[..., 1:].float()
    p = torch.sigmoid(x)
    bce = x.clamp(min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    cls = (t * 0.25 + (1 - t) * 0.75) * (t * (1.0 - p) + (1.0 - t) * p) ** 2.0 * bce * ((labels >= 0).float() / norm).unsqueeze(-1)
    # regression: smooth L1 (beta 1 / 9) with the sine of the heading difference split over both sides
    q = preds['box_preds'].view(B, -1, 7)
    a = torch.cat([q[..., :6], torch.sin(q[..., 6:7]) * torch.cos(targets[..., 6:7])], dim=-1)
    b = torch.cat([targets[..., :6], torch.cos(q[..., 6:7]) * torch.sin(targets[..., 6:7])], dim=-1)
    n = (a - b).abs()
    beta = 1.0 / 9.0
    loc = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta) * (pos.float() / norm).unsqueeze(-1)
    # direction: the bin of the box's heading against the offset, cross entropy
    rot = targets[..., 6] + anchors[None, :, 6]
    off = rot - R.HEAD_CFG['DIR_OFFSET']
    off = off - torch.floor(off / (2 * math.pi) + 0) * (2 * math.pi)
    bins = torch.floor(off / (2 * math.pi / 2)).long().clamp(0, 1)
    logits = preds['dir_cls_preds'].view(B, -1, 2)
    dirs = (torch.logsumexp(logits, dim=-1) - logits.gather(-1, bins.unsqueeze(-1)).squeeze(-1)) * (pos.float() / norm)
    l_cls, l_loc, l_dir = cls.sum() / B * w['cls_weight'], loc.sum() / B * w['loc_weight'], dirs.sum() / B * w['dir_weight']
    return {'cls': cls, 'loc': loc, 'dir': dirs}, [l_cls + l_loc + l_dir, l_cls, l_loc, l_dir]


def plain_decode(g, preds):
    import torch
    anchors = cu(g['anchors'])[None]
    q = preds['box_preds'].view(R.G25_B, -1, 7)
    diag = torch.sqrt(anchors[..., 3] ** 2 + anchors[..., 4] ** 2)
    cols = [q[..., 0] * diag + anchors[..., 0], q[..., 1] * diag + anchors[..., 1], q[..., 2] * anchors[..., 5] + anchors[..., 2],
            torch.exp(q[..., 3]) * anchors[..., 3], torch.exp(q[..., 4]) * anchors[..., 4], torch.exp(q[..., 5]) * anchors[..., 5]]
    rot = q[..., 6] + anchors[..., 6]
    label = preds['dir_cls_preds'].view(R.G25_B, -1, 2).max(dim=-1)[1]
    v = rot - R.HEAD_CFG['DIR_OFFSET']
    v = v - torch.floor(v / math.pi + R.HEAD_CFG['DIR_LIMIT_OFFSET']) * math.pi
    cols.append(v + R.HEAD_CFG['DIR_OFFSET'] + math.pi * label.float())
    return torch.stack(cols, dim=-1)


def test_head_losses_gradients_and_decoding_against_golden_g25():
    import torch
    from tests.test_anchor_target_host import head_on_golden
    g = np.load(GOLDEN)
    head = head_on_golden(g, DEV)
    ret = head.forward_ret_dict
    loss, tb = head.get_loss()
    loss.backward()
    keys = ('cls_preds', 'box_preds', 'dir_cls_preds')
    preds = {k: cu(g[k]).requires_grad_() for k in keys}
    terms, scalars = plain_losses(g, preds)
    scalars[0].backward()
    assert set(tb) == {'rpn_loss', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir'} and all(isinstance(v, float) for v in tb.values())
    for k in ('cls', 'loc', 'dir'):
        _within(k + '_loss_src', ret[k + '_loss_src'], terms[k], g[k + '_loss_src'])
    got = torch.tensor([tb[k] for k in ('rpn_loss', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir')])
    for j, k in enumerate(('rpn_loss', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir')):
        _within(k, got[j], scalars[j], g['loss'][j:j + 1].astype(np.float32))
    for k in keys:
        assert np.abs(g['grad_' + k]).max() > 0
        _within('grad ' + k, ret[k].grad, preds[k].grad, g['grad_' + k])
    with torch.no_grad():
        cls, box = head.generate_predicted_boxes(R.G25_B, ret['cls_preds'].detach(), ret['box_preds'].detach(),
                                                 ret['dir_cls_preds'].detach())
        plain = plain_decode(g, preds)
    assert tuple(cls.shape) == (3, 720, 3) and np.array_equal(cls.cpu().numpy(), g['batch_cls_preds'])
    for c, name in enumerate(('x', 'y', 'z', 'dx', 'dy', 'dz', 'heading')):
        _within('decoded ' + name, box[..., c], plain[..., c], g['batch_box_preds'][..., c])
    # the head's forward: the same three outputs from the golden's features
    head.eval()
    with torch.no_grad():
        d = head({'spatial_features_2d': cu(g['spatial_features_2d']), 'batch_size': R.G25_B})
    for k in keys:
        gold = g[k]
        err = np.abs(head.forward_ret_dict[k].cpu().numpy() - gold).max()
        assert err <= 32 * 2.0 ** -23 * max(1.0, np.abs(gold).max()), (k, err)     # 32 terms of about 1 per output
    assert d['cls_preds_normalized'] is False and tuple(d['batch_box_preds'].shape) == (3, 720, 7)


# ---- SECONDNet on a KITTI directory ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kitti_root(tmp_path_factory):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import create_kitti_infos
    root = str(tmp_path_factory.mktemp("kitti_second"))
    KC.write_kitti(root, KC.all_frames(), split='train')
    plain = kitti_cfg()
    plain['DATA_PROCESSOR'] = plain['DATA_PROCESSOR'][:1]
    create_kitti_infos(plain, KC.CLASSES, root, root, workers=2)
    return root


def dataset(root, training):
    from dfu3d_amd.pcdet_kitti.kitti_dataset import KittiDataset
    ds = KittiDataset(kitti_cfg(), R.CLASS_NAMES, training=training, root_path=root, device=DEV)
    ds.voxel_features_only = True
    return ds


def model_for(ds, seed):
    import torch
    from dfu3d_amd.pcdet_kitti.second_net import SECONDNet
    torch.manual_seed(seed)
    return SECONDNet(cfg(R.SECOND_MODEL), len(R.CLASS_NAMES), dataset=ds).to(DEV)


def test_second_net_trains_evaluates_and_reloads(kitti_root, tmp_path):
    import torch
    from dfu3d_amd.eval_utils.eval_utils import eval_one_epoch
    from dfu3d_amd.train_utils import train_utils as T
    from dfu3d_amd.train_utils.optimization import build_optimizer, build_scheduler
    from tests import optimizer_cases as OC
    ds = dataset(kitti_root, True)
    assert [int(v) for v in ds.grid_size] == [128, 96, 40] and list(ds.class_names) == R.CLASS_NAMES
    model = model_for(ds, 41).train()
    assert [type(m).__name__ for m in model.module_list] == ['MeanVFE', 'VoxelBackBone8x', 'HeightCompression',
                                                             'BaseBEVBackbone', 'AnchorHeadSingle']
    assert [tuple(a.shape) for a in model.dense_head.anchors] == [(1, 12, 16, 1, 2, 7)] * 3
    # one step by hand: the loss, the targets of the stage, the gradients of the head
    batch = next(iter(ds.batches(6)))
    ret, tb, disp = model(batch)
    ret['loss'].backward()
    torch.cuda.synchronize()
    fwd = model.dense_head.forward_ret_dict
    labels = fwd['box_cls_labels']
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (6, 1152) and tuple(fwd['box_reg_targets'].shape) == (6, 1152, 7)
    assert int((labels > 0).sum()) > 0 and torch.equal(fwd['reg_weights'], (labels > 0).float())
    want = R.assign_targets(R.generate_anchors([float(v) for v in ds.point_cloud_range], [(16, 12)] * 3)[0],
                            batch['gt_boxes'].cpu().numpy())
    assert np.array_equal(labels.cpu().numpy(), want[0])
    loss = float(ret['loss'].detach())
    assert np.isfinite(loss) and loss > 0 and set(tb) >= {'loss_rpn', 'rpn_loss', 'rpn_loss_cls', 'rpn_loss_loc', 'rpn_loss_dir'}
    assert tb['loss_rpn'] == tb['rpn_loss'] == pytest.approx(loss, rel=1e-6) and disp == {}
    for name in ('conv_cls', 'conv_box', 'conv_dir_cls'):
        for p in getattr(model.dense_head, name).parameters():
            grad = p.grad.detach().cpu().numpy()
            assert np.isfinite(grad).all() and grad.any(), name
    dead = [k for k, p in model.named_parameters() if p.grad is None or not bool(torch.isfinite(p.grad).all())]
    assert not dead, dead
    # the training loop: two iterations of three frames through the OptimWrapper
    model.zero_grad()
    loader = ds.batches(3)
    ocfg = OC.optim_cfg(PCT_START=0.5)
    opt = build_optimizer(model, ocfg)
    assert type(opt).__name__ == 'OptimWrapper'
    sched, _ = build_scheduler(opt, len(loader), 1, -1, ocfg)
    rows = []

    class Tb:
        def add_scalar(self, tag, value, step):
            rows.append((tag, float(value), step))

    class Logger:
        def info(self, msg):
            pass
    before = {k: v.detach().clone() for k, v in model.dense_head.state_dict().items()}
    T.train_model(model, opt, loader, T.model_fn_decorator(), sched, ocfg, start_epoch=0, total_epochs=1, start_iter=0, rank=0,
                  tb_log=Tb(), ckpt_save_dir=tmp_path, logger=Logger(), logger_iter_interval=1)
    losses = [v for t, v, _ in rows if t == 'train/loss']
    assert len(losses) == 2 and np.isfinite(losses).all() and int(model.global_step) == 2
    assert all(not torch.equal(v, model.dense_head.state_dict()[k]) for k, v in before.items())
    # its own checkpoint, strict
    fresh = model_for(ds, 42)
    ck = fresh.load_params_from_file(str(tmp_path / 'checkpoint_epoch_1.pth'))
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in fresh.state_dict().items()) and 'model_state' in ck
    # evaluation: one step by hand to pred_dicts, then the epoch
    ev = dataset(kitti_root, False)
    fresh.eval()
    with torch.no_grad():
        fresh.dense_head.conv_cls.bias += 3.5                         # an untrained head scores under the threshold
        pred, recall = fresh(next(iter(ev.batches(2))))
    assert len(pred) == 2 and all(set(p) >= {'pred_boxes', 'pred_scores', 'pred_labels'} for p in pred) and 'gt' in recall
    for p in pred:
        n = p['pred_scores'].shape[0]
        assert 0 < n <= 500 and tuple(p['pred_boxes'].shape) == (n, 7) and bool((p['pred_scores'] >= 0.2).all())
        assert bool(((p['pred_labels'] >= 1) & (p['pred_labels'] <= 3)).all())
    ret = eval_one_epoch(cfg({'MODEL': R.SECOND_MODEL}), Cfg(save_to_file=False), fresh, ev.batches(2), 1, Logger(),
                         result_dir=tmp_path / 'eval')
    assert all(0.0 <= ret['recall/rcnn_' + t] <= 1.0 for t in ('0.3', '0.5', '0.7'))
