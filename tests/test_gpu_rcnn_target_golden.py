"""GPU: PointRCNN's training half against golden G21 (tests/golden/capture_rcnn_target_golden.py: the reference's own
heads, target layer and losses on golden G20's model and backbone output).  The targets are computed from the model's own
forward with the golden's sampled indices; the losses, their per-element terms and their gradients from the golden's own
predictions and targets.  Every integer must be equal, every float within
d_hip <= max(4 * d_torch, 4 ulp at the golden's largest magnitude), d_torch being the deviation of the plain formulation
of tests/rcnn_target_ref.py on the same GPU (for the losses: torch primitives only, no code of the heads' loss functions)
-- the rule and the margin of golden G20."""
import json
import os

import numpy as np
import pytest

from tests import rcnn_target_ref as T
from tests import roipoint_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def cu(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _within(name, hip, plain, gold):
    hip, plain = hip.detach().cpu().numpy().reshape(gold.shape), plain.detach().cpu().numpy().reshape(gold.shape)
    d_hip, d_torch = float(np.abs(hip - gold).max()), float(np.abs(plain - gold).max())
    floor = 4.0 * float(np.spacing(np.float32(np.abs(gold).max())))
    print("G21 %-22s d_hip %.3g  d_torch %.3g  floor %.3g  (largest |golden| %.3g)" % (name, d_hip, d_torch, floor, np.abs(gold).max()))
    assert d_hip <= max(4.0 * d_torch, floor), (name, d_hip, d_torch, floor)


def _same(name, got, gold):
    got = got.detach().cpu().numpy().reshape(gold.shape)
    assert np.array_equal(got.astype(np.int64), gold.astype(np.int64)), name


def losses_on_golden(model, g, cfg, dev):
    """The heads' losses, their per-element terms and their gradients on the GOLDEN's own predictions and targets, and the
    same from the formulation of tests/rcnn_target_ref.py, which shares no code with the heads' losses -> rows
    (name, the heads' value, the plain value, the golden's) for _within.  Runs on any device."""
    import torch
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)   # noqa: E731
    head, loss_cfg = model.roi_head, cfg['ROI_HEAD']['LOSS_CONFIG']
    leaf = lambda name: to(g[name]).requires_grad_(True)               # noqa: E731
    names = ['point_cls_preds', 'point_box_preds', 'rcnn_cls', 'rcnn_reg']
    leaves = [leaf(n) for n in names]
    plain_leaves = [leaf(n) for n in names]
    stored = {k: to(g["t_" + k]) for k in ('rois', 'gt_of_rois', 'gt_of_rois_src', 'reg_valid_mask', 'rcnn_cls_labels')}
    terms, hooks = {}, []
    for owner, tag in ((model.point_head, 'point_'), (head, 'rcnn_')):
        for name in ('cls_loss_func', 'reg_loss_func'):
            if hasattr(owner, name):
                hooks.append(getattr(owner, name).register_forward_hook(
                    lambda m, i, o, key=tag + name: terms.__setitem__(key, o.detach())))
    model.point_head.forward_ret_dict = {'point_cls_preds': leaves[0], 'point_box_preds': leaves[1],
                                         'point_cls_labels': to(g["point_cls_labels"]), 'point_box_labels': to(g["point_box_labels"])}
    head.forward_ret_dict = dict({k: v.clone() for k, v in stored.items()}, rcnn_cls=leaves[2], rcnn_reg=leaves[3])
    loss, tb, _ = model.get_training_loss(as_tensors=True)
    for h in hooks:
        h.remove()
    weights = cfg['POINT_HEAD']['LOSS_CONFIG']['LOSS_WEIGHTS']
    pp = T.plain_point_losses(plain_leaves[0], plain_leaves[1], to(g["point_cls_labels"]), to(g["point_box_labels"]), 3, weights,
                              weights['code_weights'])
    pr = T.plain_rcnn_losses(dict(stored, rcnn_cls=plain_leaves[2], rcnn_reg=plain_leaves[3]), head.box_coder.code_size, loss_cfg)
    assert float(tb['point_pos_num']) == float(g["loss_point_pos_num"]) == float(pp['point_pos_num'])
    rows = [(k, tb[k], pp[k], np.float32(g["loss_" + k])) for k in ('point_loss_cls', 'point_loss_box')]
    rows += [(k, tb[k], pr[k], np.float32(g["loss_" + k])) for k in ('rcnn_loss_cls', 'rcnn_loss_reg', 'rcnn_loss_corner', 'rcnn_loss')]
    rows += [("terms point cls", terms['point_cls_loss_func'], pp['cls_terms'], g["terms_point_cls_loss_func"]),
             ("terms point box", terms['point_reg_loss_func'], pp['box_terms'], g["terms_point_reg_loss_func"]),
             ("terms rcnn reg", terms['rcnn_reg_loss_func'], pr['reg_terms'], g["terms_rcnn_reg_loss_func"])]
    got = torch.autograd.grad(loss, leaves)
    want = torch.autograd.grad(pp['point_loss_cls'] + pp['point_loss_box'] + pr['rcnn_loss'], plain_leaves)
    return rows + [("grad " + n, a, b, g["grad_" + n]) for n, a, b in zip(names, got, want)]


def g21_model(golden_dir):
    """-> (the trainable model with golden G20's weights, on the CPU, in training mode; golden G21; its configuration)."""
    import torch
    from dfu3d_amd.pcdet_kitti.point_rcnn import PointRCNN
    g20 = dict(np.load(os.path.join(golden_dir, "g20_pointrcnn.npz")))
    g = dict(np.load(os.path.join(golden_dir, "g21_pointrcnn_train.npz")))
    cfg = R.g20_model_cfg()
    cfg['ROI_HEAD']['TARGET_CONFIG']['ROI_PER_IMAGE'] = json.loads(bytes(g["meta"]).decode())['roi_per_image']
    model = PointRCNN(cfg, len(R.G20_CLASSES), class_names=R.G20_CLASSES, num_point_features=3 + R.G20_EXTRA, trainable=True)
    keys = json.loads(bytes(g20["meta"]).decode())["state_dict_keys"]
    model.load_state_dict({k: torch.from_numpy(g20["sd_" + k].copy()) for k in keys}, strict=True)
    return model.train(), g, g20, cfg


def test_g21_targets_losses_and_gradients(golden_dir):
    import torch
    model, g, g20, cfg = g21_model(golden_dir)
    model = model.to(DEV)
    sampler = cfg['ROI_HEAD']['TARGET_CONFIG']
    gt = cu(g["gt_boxes"])
    d = dict(batch_size=R.G20_B, point_features=cu(g20["point_features"]), point_coords=cu(g20["point_coords"]), gt_boxes=gt)
    # ---- the first stage: targets -------------------------------------------------------------------------------------
    d = model.point_head(d)
    p = model.point_head.forward_ret_dict
    assert torch.equal(gt, cu(g["gt_boxes"]))                                          # gt_boxes is not written
    _same("point_cls_labels", p['point_cls_labels'], g["point_cls_labels"])
    plain_cls, plain_box = T.plain_point_targets(d['point_coords'], gt, cfg['POINT_HEAD']['TARGET_CONFIG']['GT_EXTRA_WIDTH'], 3,
                                                 model.point_head.box_coder)
    _same("plain point_cls_labels", plain_cls, g["point_cls_labels"])
    _within("point_box_labels", p['point_box_labels'], plain_box, g["point_box_labels"])
    # ---- the second stage: proposals, targets (the steps of the training forward, with the golden's sampled indices) ----
    head = model.roi_head
    head.proposal_layer(d, nms_config=cfg['ROI_HEAD']['NMS_CONFIG']['TRAIN'])
    rois_all, labels_all, scores_all = d['rois'].clone(), d['roi_labels'].clone(), d['roi_scores'].clone()
    _same("roi_labels_all", labels_all, g["roi_labels_all"])
    r = head.assign_targets(d, sampled_inds=cu(g["sampled_inds"]))
    plain = T.plain_roi_targets(T.plain_proposal_targets(rois_all, scores_all, labels_all, gt, sampler, cu(g["sampled_inds"]),
                                                         T.gpu_iou3d), R.G20_B)
    _same("sampled_inds", r['sampled_inds'], g["sampled_inds"])
    _same("gt_assignment", r['gt_assignment'], g["gt_assignment"])
    _within("max_overlaps", r['max_overlaps'], plain['max_overlaps'], g["max_overlaps"])
    for k in ('roi_labels', 'reg_valid_mask', 'rcnn_cls_labels'):
        assert r[k].dtype == torch.int64
        _same(k, r[k], g["t_" + k])
        _same("plain " + k, plain[k], g["t_" + k])
    for k in ('rois', 'gt_of_rois', 'gt_of_rois_src', 'gt_iou_of_rois', 'roi_scores'):
        _within(k, r[k], plain[k], g["t_" + k])
    head.proposal_target_layer.check_status()
    for row in losses_on_golden(model, g, cfg, DEV):
        _within(*row)
