"""PointRCNN's target assignment and training half without a GPU: the agreement of include/dfu3d_tgt.h with its binding,
host-side argument validation before any launch, the sequential restatements of the three kernels against the plain
formulation in the reference's shape (tests/rcnn_target_ref.py), and the trainable model's construction."""
import ctypes
import os

import numpy as np
import pytest

from dfu3d_amd import _build, _lib, _lib_tgt
from tests import rcnn_target_ref as T
from tests import roipoint_ref as R

P16 = ctypes.c_void_p(16)            # a non-null, 16-byte aligned address no call may touch
SYMBOLS = ['dfu3d_tgt_point_targets', 'dfu3d_tgt_roi_max_iou', 'dfu3d_tgt_roi_sample', 'dfu3d_tgt_version']
OTHER_PREFIXES = ('dfu3d_vfe', 'dfu3d_head', 'dfu3d_post', 'dfu3d_aug', 'dfu3d_bev', 'dfu3d_opt', 'dfu3d_ingest',
                  'dfu3d_pn2', 'dfu3d_roi')


def test_header_and_binding_agree():
    assert _lib_tgt.HEADER == os.path.join(_build.INCLUDE, "dfu3d_tgt.h") and _lib_tgt.HEADER in _build._deps()
    assert _lib_tgt.header_symbols() == SYMBOLS
    L = _lib_tgt.lib()
    assert all(hasattr(L, s) for s in SYMBOLS)
    assert L.dfu3d_tgt_version() == _lib_tgt.header_version() == 1
    K = _lib_tgt.CONSTANTS
    assert all(k.startswith("DFU3D_TGT_") for k in K)
    assert K['DFU3D_TGT_MAX_ELEMS'] == 2 ** 31 - 1 and K['DFU3D_TGT_MAX_BATCH'] == 65535
    assert (K['DFU3D_TGT_MAX_ROIS'], K['DFU3D_TGT_MAX_SAMPLED'], K['DFU3D_TGT_MAX_CLASSES']) == (2048, 4096, 64)
    assert K['DFU3D_TGT_POINT_LAUNCHES'] == K['DFU3D_TGT_IOU_LAUNCHES'] == K['DFU3D_TGT_SAMPLE_LAUNCHES'] == 1
    assert K['DFU3D_TGT_STATUS_NO_ROI'] == 1
    res, args = _lib_tgt.SIGNATURES['dfu3d_tgt_point_targets']
    assert res is ctypes.c_int32 and len(args) == 16 and args[-1] is ctypes.c_void_p and args[9:12] == [ctypes.c_float] * 3
    res, args = _lib_tgt.SIGNATURES['dfu3d_tgt_roi_max_iou']
    assert res is ctypes.c_int32 and len(args) == 10 and args[3:7] == [ctypes.c_int32] * 4
    res, args = _lib_tgt.SIGNATURES['dfu3d_tgt_roi_sample']
    assert res is ctypes.c_int32 and len(args) == 14 and args[7:10] == [ctypes.c_float] * 3 and args[10] is ctypes.c_double
    assert _lib_tgt.SIGNATURES['dfu3d_tgt_version'] == (ctypes.c_int32, [])
    assert not set(_lib_tgt.SIGNATURES) & set(_lib.SIGNATURES)
    own = open(_lib_tgt.HEADER).read()
    headers = sorted(os.listdir(_build.INCLUDE))
    assert "dfu3d_tgt.h" in headers and "dfu3d.h" in headers and "dfu3d_roi.h" in headers
    assert sorted("dfu3d_" + h[len("dfu3d_"):-2] for h in headers if h not in ("dfu3d.h", "dfu3d_tgt.h")) == sorted(OTHER_PREFIXES)
    for prefix in OTHER_PREFIXES:
        assert prefix not in own and prefix.upper() not in own, prefix
    for other in headers:
        if other != "dfu3d_tgt.h":
            text = open(os.path.join(_build.INCLUDE, other)).read()
            assert "dfu3d_tgt" not in text and "DFU3D_TGT" not in text, other
    from dfu3d_amd import rcnn_target_ops as ops
    assert (ops.POINT_LAUNCHES, ops.IOU_LAUNCHES, ops.SAMPLE_LAUNCHES, ops.MAX_ROIS, ops.MAX_SAMPLED) == (1, 1, 1, 2048, 4096)


def test_binding_names_a_missing_symbol():
    class Fake:
        _name = "fake.so"
    Fake.dfu3d_tgt_version = object()
    with pytest.raises(_lib.Dfu3dError, match="fake.so does not export dfu3d_tgt_point_targets, dfu3d_tgt_roi_max_iou"):
        _lib_tgt.bind(Fake())


def _points(L, pts=P16, stride=4, gt=P16, mean=P16, B=2, N=64, G=5, K=3, nc=3, ex=0.2, ey=0.2, ez=0.2,
            cls=ctypes.c_void_p(32), box=ctypes.c_void_p(48), idx=ctypes.c_void_p(64)):
    return L.dfu3d_tgt_point_targets(pts, stride, gt, mean, B, N, G, K, nc, ex, ey, ez, cls, box, idx, None)


def _iou(L, rois=P16, labels=P16, gt=P16, B=2, M=12, G=5, by_class=1, ov=ctypes.c_void_p(32), asg=ctypes.c_void_p(48)):
    return L.dfu3d_tgt_roi_max_iou(rois, labels, gt, B, M, G, by_class, ov, asg, None)


def _sample(L, ov=P16, key=P16, u=P16, B=2, M=12, R_=8, fg_per=4, fg=0.55, reg=0.55, lo=0.1, ratio=0.8,
            out=ctypes.c_void_p(32), status=ctypes.c_void_p(48)):
    return L.dfu3d_tgt_roi_sample(ov, key, u, B, M, R_, fg_per, fg, reg, lo, ratio, out, status, None)


def test_bad_arguments_return_before_any_launch():
    """Every call below passes pointers no kernel may touch: a launch would fault (or, without a GPU, fail with
    DFU3D_ELAUNCH); each must come back with the validation's own code."""
    L = _lib_tgt.lib()
    EINVAL, ERANGE = _lib.CONSTANTS["DFU3D_EINVAL"], _lib.CONSTANTS["DFU3D_ERANGE"]
    K = _lib_tgt.CONSTANTS
    for name in ('pts', 'gt', 'cls', 'box'):
        assert _points(L, **{name: None}) == EINVAL, name
    assert _points(L, mean=None) == EINVAL and _points(L, K=0) == EINVAL          # mean sizes and their count go together
    for name in ('B', 'N', 'G', 'nc'):
        assert _points(L, **{name: 0}) == EINVAL and _points(L, **{name: -1}) == EINVAL, name
    assert _points(L, K=-1) == EINVAL and _points(L, stride=2) == EINVAL and _points(L, stride=65) == EINVAL
    assert _points(L, box=ctypes.c_void_p(40)) == EINVAL                           # box_labels not on 16 bytes
    assert _points(L, ex=float('nan')) == EINVAL
    assert _points(L, B=4, N=2 ** 26) == ERANGE                                    # B * N * 8
    assert _points(L, B=65535, N=1, G=4097) == ERANGE                              # B * G * 8
    assert _points(L, B=K['DFU3D_TGT_MAX_BATCH'] + 1, N=1, G=1) == ERANGE
    assert _points(L, K=K['DFU3D_TGT_MAX_CLASSES'] + 1) == ERANGE
    for name in ('rois', 'labels', 'gt', 'ov', 'asg'):
        assert _iou(L, **{name: None}) == EINVAL, name
    for name in ('B', 'M', 'G'):
        assert _iou(L, **{name: 0}) == EINVAL and _iou(L, **{name: -1}) == EINVAL, name
    assert _iou(L, by_class=2) == EINVAL and _iou(L, by_class=-1) == EINVAL
    assert _iou(L, B=65535, M=4682) == ERANGE and _iou(L, B=65535, G=4097) == ERANGE
    assert _iou(L, B=K['DFU3D_TGT_MAX_BATCH'] + 1, M=1, G=1) == ERANGE
    for name in ('ov', 'key', 'u', 'out', 'status'):
        assert _sample(L, **{name: None}) == EINVAL, name
    for name in ('B', 'M', 'R_'):
        assert _sample(L, **{name: 0}) == EINVAL and _sample(L, **{name: -1}) == EINVAL, name
    assert _sample(L, fg_per=-1) == EINVAL and _sample(L, fg_per=9) == EINVAL
    for ratio in (-0.1, 1.1, float('nan')):
        assert _sample(L, ratio=ratio) == EINVAL, ratio
    assert _sample(L, M=K['DFU3D_TGT_MAX_ROIS'] + 1) == ERANGE
    assert _sample(L, R_=K['DFU3D_TGT_MAX_SAMPLED'] + 1, fg_per=4) == ERANGE
    assert _sample(L, B=K['DFU3D_TGT_MAX_BATCH'] + 1) == ERANGE


@pytest.mark.parametrize("use_mean", [True, False])
def test_point_target_restatement_matches_the_plain_formulation(use_mean):
    import torch
    from dfu3d_amd.pcdet_kitti import box_coder_utils as bc
    pts, gt = T.random_point_case(11, 3, 97, 6)
    gt[0, 2, 7] = 0                                           # a class-0 row: its points are background
    gt[1, 4:] = 0                                             # padded rows
    pts[1, 5] = [0.0, 0.0, 0.0]
    pts[1, 6] = [0.05, 0.0, 0.0]
    extra = (0.2, 0.2, 0.2)
    for num_class in (3, 1):
        cls, box, idx = T.point_targets(pts, gt, extra, num_class, T.MEAN_SIZE if use_mean else None)
        coords = np.concatenate([np.repeat(np.arange(3), 97)[:, None].astype(np.float32), pts.reshape(-1, 3)], axis=1)
        coder = bc.PointResidualCoder(use_mean_size=use_mean, mean_size=T.MEAN_SIZE)
        before = gt.copy()
        pcls, pbox = T.plain_point_targets(torch.from_numpy(coords), torch.from_numpy(gt), list(extra), num_class, coder)
        assert np.array_equal(gt, before)
        assert np.array_equal(cls, pcls.numpy())
        assert (cls > 0).sum() > 40 and (cls == -1).sum() > 3 and (cls == 0).sum() > 40
        # the origin is INSIDE the first zero row (|0| < 0 + 1e-5): a hit on a class-0 row, background; 0.05 m away
        # only the enlarged zero box holds the point: ignored
        assert (cls[97 + 5], idx[97 + 5]) == (0, 4) and (cls[97 + 6], idx[97 + 6]) == (-1, -1)
        assert (cls[idx < 0] <= 0).all() and (cls[idx >= 0] >= 0).all()
        hit0 = (idx[:97] == 2)
        assert hit0.any() and (cls[:97][hit0] == 0).all() and not box[:97][hit0].any()
        assert np.allclose(box, pbox.numpy(), rtol=0, atol=4 * np.spacing(np.float32(np.abs(box).max())))
        assert not box[cls <= 0].any()


@pytest.mark.parametrize("by_class", [True, False])
def test_max_iou_restatement_matches_the_plain_formulation(by_class):
    import torch
    rng = np.random.default_rng(5)
    gt = T.random_boxes(rng, 3, 7)
    gt[0, 5:] = 0                                             # trailing zero rows
    gt[1, 2] = 0                                              # an interleaved zero row
    gt[2] = 0                                                 # a sample without boxes
    gt[0, 1] = gt[0, 0]                                       # two identical rows: the lower index wins
    gt[1, :, 7] = np.where(gt[1, :, 7] == 3, 1, gt[1, :, 7])  # no box of class 3 in sample 1
    rois, labels = T.jittered_rois(rng, gt, 21)
    rois[0, 3], labels[0, 3] = gt[0, 1, :7], int(gt[0, 1, 7])
    labels[1, :4] = 3
    rois[1, 20] = 0                                           # a zero-padded RoI
    iou = np.stack([T.numpy_iou3d(rois[b], gt[b, :, :7]) for b in range(3)])
    ov, asg = T.max_iou(iou, labels, gt, by_class)
    pov, pasg = T.plain_max_iou(torch.from_numpy(rois), torch.from_numpy(labels), torch.from_numpy(gt), by_class, T.cpu_iou3d)
    assert np.array_equal(ov, pov.numpy()) and np.array_equal(asg, pasg.numpy())
    assert asg[0, 3] == 0 and ov[0, 3] > 0.99 and not ov[2].any() and not asg[2].any()
    if by_class:
        assert not ov[1, :4].any() and not asg[1, :4].any()
    assert (ov > 0.55).sum() > 5 and ((ov > 0) & (ov < 0.55)).sum() > 3


def sampler_rows():
    """max_overlaps rows (M = 12) that take every branch of the sampler with ROI_PER_IMAGE = 8, FG_RATIO = 0.5."""
    fg, hard, easy, nan = 0.8, 0.3, 0.02, float('nan')
    return np.array([
        [fg] * 2 + [hard] * 5 + [easy] * 5,                   # take < fg_per, h = int(6 * 0.8) = 4
        [fg] * 6 + [hard] * 2 + [easy] * 4,                   # take = fg_per, h clipped by nh = 2
        [fg] * 5 + [hard] * 7,                                # only hard background
        [fg] * 5 + [easy] * 7,                                # only easy background
        [fg] * 12,                                            # foreground only: draws with replacement
        [hard] * 6 + [easy] * 6,                              # background only
        [hard] * 12, [easy] * 12,
        [nan] * 12,                                           # no list at all: zeros and the status bit
        [fg, nan, hard, nan, easy, nan, fg, nan, hard, nan, easy, fg],
    ], np.float32)


def test_sampling_restatement_matches_the_plain_formulation():
    import torch
    cfg = dict(T.SAMPLER, ROI_PER_IMAGE=8)
    ov = sampler_rows()
    rng = np.random.default_rng(3)
    key = rng.integers(0, 4, ov.shape).astype(np.int32)       # few values: equal keys fall back on the index
    u = rng.uniform(0, 1, (len(ov), 8)).astype(np.float32)
    u[:, 0], u[:, 7] = 0.0, np.nextafter(np.float32(1), np.float32(0))
    out, status, parts = T.subsample(ov, cfg, key, u)
    assert status == 1 and [p[0] for p in parts] == ['both'] * 4 + ['fg_only'] + ['bg_only'] * 3 + ['none', 'both']
    assert parts[0][1:] == (2, 4) and parts[1][1:] == (4, 2) and parts[5][1:] == (0, 6) and not out[8].any()
    plain = T.plain_subsample(torch.from_numpy(ov), cfg, torch.from_numpy(key), torch.from_numpy(u))
    assert np.array_equal(out, plain.numpy())
    for b, (kind, take, h) in enumerate(parts):
        fg, hard, easy = T.lists_of(ov[b], cfg)
        if kind == 'both':
            assert set(out[b, :take]) <= set(fg) and len(set(out[b, :take])) == take
            assert set(out[b, take:take + h]) <= set(hard) and set(out[b, take + h:]) <= set(easy if easy else hard)
    assert out[4, 0] == 0 and out[4, 7] == 11                 # rand_u = 0 and the largest float below 1


def test_trainable_model_keeps_the_state_dict_and_says_what_it_lacks(tmp_path):
    import torch
    from dfu3d_amd.pcdet_kitti.point_rcnn import PointRCNN
    from dfu3d_amd.pcdet_kitti.proposal_target_layer import ProposalTargetLayer
    plain = PointRCNN(R.g20_model_cfg(), 3, class_names=R.G20_CLASSES, num_point_features=4)
    model = PointRCNN(R.g20_model_cfg(), 3, class_names=R.G20_CLASSES, num_point_features=4, trainable=True)
    assert not plain.trainable and not plain.point_head.trainable and not plain.roi_head.trainable
    assert model.trainable and model.point_head.trainable and model.roi_head.trainable
    assert isinstance(model.roi_head.proposal_target_layer, ProposalTargetLayer) and not hasattr(plain.roi_head, 'proposal_target_layer')
    keys = [(k, tuple(v.shape)) for k, v in plain.state_dict().items()]
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == keys
    assert not list(model.roi_head.proposal_target_layer.state_dict()) and not list(model.point_head.cls_loss_func.state_dict())
    path = str(tmp_path / "ckpt.pth")
    torch.save({'model_state': model.state_dict()}, path)
    plain.load_state_dict(torch.load(path)['model_state'], strict=True)
    model.load_state_dict(plain.state_dict(), strict=True)
    with pytest.raises(RuntimeError, match="run forward in training mode"):
        model.point_head.get_loss()
    with pytest.raises(RuntimeError, match="run forward in training mode"):
        model.roi_head.get_loss()
    with pytest.raises(RuntimeError, match="run forward in training mode"):
        model.get_training_loss()
    full = PointRCNN(R.full_model_cfg(), len(R.FULL_CLASSES), class_names=R.FULL_CLASSES, num_point_features=4, trainable=True)
    assert len(full.state_dict()) == 309


def test_losses_match_the_reference_formulas_on_the_cpu():
    """The masked-sum losses of PointRCNNHead against the `[fg_mask]` / `fg_sum > 0` formulation, values and gradients;
    with and without a foreground RoI."""
    import torch
    from dfu3d_amd.pcdet_kitti.point_rcnn import PointRCNN
    model = PointRCNN(R.g20_model_cfg(), 3, class_names=R.G20_CLASSES, num_point_features=4, trainable=True)
    head, rng = model.roi_head, np.random.default_rng(8)
    gt = T.random_boxes(rng, 2, 4)
    rois, labels = T.jittered_rois(rng, gt, 12)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))     # noqa: E731
    for some_fg in (True, False):
        iou_fn = T.cpu_iou3d if some_fg else (lambda a, b: T.cpu_iou3d(a, b) * 0)
        inds = t(rng.integers(0, 12, (2, 8)))
        targets = T.plain_proposal_targets(t(rois), t(rng.uniform(0, 1, (2, 12)).astype(np.float32)), t(labels), t(gt),
                                           T.SAMPLER, inds, iou_fn)
        assert bool(targets['reg_valid_mask'].any()) == some_fg
        ret = T.plain_roi_targets(targets, 2)
        got, want = {}, {}
        for out, plain in ((got, False), (want, True)):
            cls = torch.linspace(-2, 2, 16).view(16, 1).clone().requires_grad_(True)
            reg = (0.05 * torch.sin(torch.arange(16 * 7).float())).view(16, 7).clone().requires_grad_(True)
            r = dict({k: (v.clone() if torch.is_tensor(v) else v) for k, v in ret.items()}, rcnn_cls=cls, rcnn_reg=reg)
            if plain:
                terms = T.plain_rcnn_losses(r, head.box_coder.code_size, R.g20_model_cfg()['ROI_HEAD']['LOSS_CONFIG'])
                terms.pop('reg_terms')
            else:
                head.forward_ret_dict = r
                loss, tb = head.get_loss(as_tensors=True)
                terms = dict(tb)
                assert sorted(tb) == ['rcnn_loss', 'rcnn_loss_cls', 'rcnn_loss_corner', 'rcnn_loss_reg']
                terms['rcnn_loss'] = loss
            terms['rcnn_loss'].backward()
            out.update({k: float(v) for k, v in terms.items()}, cls_grad=cls.grad.clone(), reg_grad=reg.grad.clone())
        for k in ('rcnn_loss', 'rcnn_loss_cls', 'rcnn_loss_corner', 'rcnn_loss_reg'):
            assert got[k] == pytest.approx(want[k], rel=1e-5, abs=1e-7), k
        assert (got['rcnn_loss_reg'] > 0) == some_fg and (got['rcnn_loss_corner'] > 0) == some_fg
        assert torch.allclose(got['cls_grad'], want['cls_grad'], rtol=1e-5, atol=1e-8)
        assert torch.allclose(got['reg_grad'], want['reg_grad'], rtol=1e-4, atol=1e-7)


def test_g21_losses_terms_and_gradients_on_the_cpu(golden_dir):
    """The heads' losses on golden G21's own predictions and targets, on the CPU, against the golden (the reference's own
    loss code on the same inputs): the GPU test's rule, d_heads <= max(4 * d_plain, 4 ulp at the golden's largest
    magnitude), with the plain formulation that shares no code with the heads' losses."""
    from tests.test_gpu_rcnn_target_golden import _within, g21_model, losses_on_golden
    model, g, _, cfg = g21_model(golden_dir)
    rows = losses_on_golden(model, g, cfg, "cpu")
    assert len(rows) == 13
    for row in rows:
        _within(*row)


def test_an_ignored_roi_costs_nothing_by_hand():
    """rcnn_cls_labels == -1, which golden G21 cannot hold (the reference's own loss refuses that target on the CPU): the
    second stage's classification loss against numbers worked out with math.log alone, for both CLS_LOSS kinds."""
    import math
    import torch
    from dfu3d_amd.pcdet_kitti.point_rcnn import PointRCNN
    logits = [1.5, -0.5, 2.0, 0.25, -3.0, 0.0]
    labels = [1, 0, -1, 1, -1, 0]
    softplus = lambda v: math.log1p(math.exp(v))                       # noqa: E731    -log(1 - sigmoid(v))
    want = sum(softplus(-x) if y == 1 else softplus(x) for x, y in zip(logits, labels) if y >= 0) / 4
    cfg = R.g20_model_cfg()
    head = PointRCNN(cfg, 3, class_names=R.G20_CLASSES, num_point_features=4, trainable=True).roi_head
    x = torch.tensor(logits).view(6, 1).requires_grad_(True)
    loss, tb = head.get_box_cls_layer_loss({'rcnn_cls': x, 'rcnn_cls_labels': torch.tensor(labels).view(2, 3)})
    assert float(loss) == pytest.approx(want, rel=1e-6) and float(tb['rcnn_loss_cls']) == pytest.approx(want, rel=1e-6)
    loss.backward()
    sig = lambda v: 1 / (1 + math.exp(-v))                             # noqa: E731
    grad = [((sig(a) - b) / 4 if b >= 0 else 0.0) for a, b in zip(logits, labels)]
    assert x.grad.view(-1).tolist() == pytest.approx(grad, rel=1e-5, abs=1e-9) and x.grad[2, 0] == 0 and x.grad[4, 0] == 0
    cfg['ROI_HEAD']['LOSS_CONFIG']['CLS_LOSS'] = 'CrossEntropy'
    head = PointRCNN(cfg, 3, class_names=R.G20_CLASSES, num_point_features=4, trainable=True).roi_head
    two = torch.tensor([[0.0, v] for v in logits]).requires_grad_(True)             # class 1 against class 0: the same numbers
    loss, _ = head.get_box_cls_layer_loss({'rcnn_cls': two, 'rcnn_cls_labels': torch.tensor(labels)})
    assert float(loss) == pytest.approx(want, rel=1e-6)
    loss.backward()
    assert not two.grad[2].any() and not two.grad[4].any()
