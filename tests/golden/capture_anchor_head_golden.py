"""Golden G25: the reference's own anchor head -- AnchorGenerator, AxisAlignedTargetAssigner, AnchorHeadSingle over
AnchorHeadTemplate with its three losses and its box decoding -- run on the CPU.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_anchor_head_golden.py REFERENCE_ROOT      ->  tests/golden/g25_anchor_head.npz

Imported UNMODIFIED as members of a package skeleton: pcdet/models/dense_heads/target_assigner/anchor_generator.py,
axis_aligned_target_assigner.py and atss_target_assigner.py, pcdet/models/dense_heads/anchor_head_template.py and
anchor_head_single.py, pcdet/utils/box_coder_utils.py, loss_utils.py, box_utils.py and common_utils.py,
pcdet/ops/iou3d_nms/iou3d_nms_utils.py and pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py.

Stand-ins, written here: the extension modules `iou3d_nms_cuda` and `roiaware_pool3d_cuda` (empty: nothing on this path
calls them), an empty `SharedArray`, and `Tensor.cuda` mapped to the identity.

The fixture (tests/anchor_target_ref.py: G25_*): the three classes of second_ps.yaml over a feature map of 12 x 10, B = 3
-- a sample with boxes of every class and trailing zero rows, one with an interior zero row and a class without a box,
one without any box -- seeded head weights and seeded spatial_features_2d.  Stored: the anchors, the targets, the three
loss terms with their per-element sources, the gradients with respect to the head's three outputs, the decoded boxes and
the head's state-dict keys.  The IoU is float32 arithmetic of correctly rounded operations only, so labels and weights
are the same on every device; nothing here needs a margin."""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from tests import anchor_target_ref as R  # noqa: E402


class Cfg(dict):
    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key)


def to_cfg(d):
    if isinstance(d, dict):
        return Cfg({k: to_cfg(v) for k, v in d.items()})
    return [to_cfg(v) for v in d] if isinstance(d, (list, tuple)) else d


def _np(t):
    return t.detach().numpy().copy()


def load_reference():
    for name in ('pcdet', 'pcdet.utils', 'pcdet.ops', 'pcdet.ops.iou3d_nms', 'pcdet.ops.roiaware_pool3d', 'pcdet.models',
                 'pcdet.models.dense_heads', 'pcdet.models.dense_heads.target_assigner'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        if '.' in name:
            setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)
    sys.modules['SharedArray'] = types.ModuleType('SharedArray')
    for name in ('pcdet.ops.iou3d_nms.iou3d_nms_cuda', 'pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda'):
        m = types.ModuleType(name)
        sys.modules[name] = m
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)
    torch.Tensor.cuda = lambda self, *a, **k: self

    def load(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, name.replace('.', '/') + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)
        return mod
    for name in ('pcdet.utils.common_utils', 'pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils', 'pcdet.utils.box_utils',
                 'pcdet.ops.iou3d_nms.iou3d_nms_utils', 'pcdet.utils.loss_utils', 'pcdet.utils.box_coder_utils',
                 'pcdet.models.dense_heads.target_assigner.anchor_generator',
                 'pcdet.models.dense_heads.target_assigner.atss_target_assigner',
                 'pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner',
                 'pcdet.models.dense_heads.anchor_head_template'):
        load(name)
    return load('pcdet.models.dense_heads.anchor_head_single')


def make_boxes(rng):
    """(B, M, 8): boxes of about their class's anchor size, inside the 9.6 m x 8 m range."""
    sizes = {1: (3.9, 1.6, 1.56, -1.0), 2: (0.8, 0.6, 1.73, 0.27), 3: (1.76, 0.6, 1.73, 0.27)}

    def box(c):
        dx, dy, dz, z = sizes[c]
        s = rng.uniform(0.85, 1.15, 3)
        h = rng.choice([0.0, 1.57, -1.57, 3.1]) + rng.uniform(-0.3, 0.3)
        return [rng.uniform(1.0, 8.6), rng.uniform(-3.2, 3.2), z + rng.uniform(-0.2, 0.2), dx * s[0], dy * s[1], dz * s[2], h, c]
    gt = np.zeros((R.G25_B, R.G25_M, 8), np.float32)
    gt[0, :6] = np.array([box(c) for c in (1, 2, 3, 2, 1, 3)], np.float32)          # three trailing zero rows
    gt[1, 0] = box(2)
    gt[1, 2] = box(1)                                                                # row 1 an interior zero row; no Bicycle
    return gt                                                                         # sample 2: no box at all


def main():
    ahs = load_reference()
    rng = np.random.default_rng(R.G25_SEED)
    torch.manual_seed(R.G25_SEED)
    torch.set_num_threads(1)
    head = ahs.AnchorHeadSingle(model_cfg=to_cfg(R.HEAD_CFG), input_channels=R.G25_CHANNELS, num_class=len(R.CLASS_NAMES),
                                class_names=R.CLASS_NAMES, grid_size=np.array(R.G25_GRID), point_cloud_range=R.G25_RANGE,
                                predict_boxes_when_training=True)
    with torch.no_grad():
        for name, p in head.named_parameters():
            if name.endswith('weight'):
                std = 0.2 if name == 'conv_box.weight' else 1.0
                p.copy_(torch.from_numpy(rng.normal(0, std / np.sqrt(R.G25_CHANNELS), tuple(p.shape)).astype(np.float32)))
            elif name != 'conv_cls.bias':                                            # conv_cls.bias keeps the reference's init
                p.copy_(torch.from_numpy(rng.normal(0, 0.1, tuple(p.shape)).astype(np.float32)))
    head.train()
    ny, nx = R.G25_GRID[1] // 8, R.G25_GRID[0] // 8
    feats = rng.normal(0, 1, (R.G25_B, R.G25_CHANNELS, ny, nx)).astype(np.float32)
    gt = make_boxes(rng)
    src = {}
    for key, fn in (('cls', head.cls_loss_func), ('loc', head.reg_loss_func), ('dir', head.dir_loss_func)):
        fn.register_forward_hook(lambda m, i, o, key=key: src.__setitem__(key, _np(o)))
    d = head({'spatial_features_2d': torch.from_numpy(feats.copy()), 'gt_boxes': torch.from_numpy(gt.copy()),
              'batch_size': R.G25_B})
    ret = head.forward_ret_dict
    for k in ('cls_preds', 'box_preds', 'dir_cls_preds'):
        ret[k].retain_grad()
    out = {'spatial_features_2d': feats, 'gt_boxes': gt}
    for k, a in enumerate(head.anchors):
        out['anchors%d' % k] = _np(a)
    out['anchors'] = _np(torch.cat(head.anchors, dim=-3).view(-1, 7))
    out['box_cls_labels'], out['box_reg_targets'] = _np(ret['box_cls_labels']), _np(ret['box_reg_targets'])
    out['reg_weights'] = _np(ret['reg_weights'])
    assert out['box_cls_labels'].dtype == np.int32 and (out['box_cls_labels'] > 0).any(1).tolist() == [True, True, False]
    assert set(np.unique(out['box_cls_labels'][0])) == {-1, 0, 1, 2, 3}
    loss, tb = head.get_loss()
    loss.backward()
    out['loss'] = np.array([tb['rpn_loss'], tb['rpn_loss_cls'], tb['rpn_loss_loc'], tb['rpn_loss_dir']], np.float64)
    out['loss_f32'] = _np(loss).reshape(1)
    out['cls_loss_src'], out['loc_loss_src'], out['dir_loss_src'] = src['cls'], src['loc'], src['dir']
    for k in ('cls_preds', 'box_preds', 'dir_cls_preds'):
        out[k], out['grad_' + k] = _np(ret[k]), _np(ret[k].grad)
    out['batch_cls_preds'], out['batch_box_preds'] = _np(d['batch_cls_preds']), _np(d['batch_box_preds'])
    sd = head.state_dict()
    for k, v in sd.items():
        out['sd_' + k] = _np(v)
    meta = {'torch': torch.__version__, 'seed': R.G25_SEED, 'state_dict_keys': [[k, list(v.shape)] for k, v in sd.items()],
            'num_anchors_per_location': int(head.num_anchors_per_location), 'classes': R.CLASS_NAMES}
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'g25_anchor_head.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'positives per sample:', (out['box_cls_labels'] > 0).sum(1).tolist(), 'loss', tb)


if __name__ == '__main__':
    main()
