"""Golden G27: the reference's own AxisAlignedTargetAssigner, alone, at a layout that is not KITTI's -- five class names,
three anchor classes in an order that is not the class order (Cyclist, Car, Truck: ids 3, 1, 5), 1, 2 and 1 sizes with three
rotations each (sets of 3, 6 and 3 slots), dyadic thresholds with unmatched == matched in the first set -- run on the CPU.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_anchor_assigner_golden.py REFERENCE_ROOT      ->  tests/golden/g27_anchor_assigner.npz

Imported UNMODIFIED as members of a package skeleton: pcdet/models/dense_heads/target_assigner/anchor_generator.py and
axis_aligned_target_assigner.py, pcdet/utils/box_coder_utils.py, box_utils.py and common_utils.py,
pcdet/ops/iou3d_nms/iou3d_nms_utils.py and pcdet/ops/roiaware_pool3d/roiaware_pool3d_utils.py.

Stand-ins, written here: the extension modules `iou3d_nms_cuda` and `roiaware_pool3d_cuda` (empty: nothing on this path
calls them), an empty `SharedArray`, and `Tensor.cuda` mapped to the identity.

The fixture (tests/anchor_target_ref.py: G27_*, g27_boxes): 17 x 17 locations 2 m apart, 3 468 anchors of 2 x 2, 1 x 2 and
1 x 1 metres on dyadic coordinates, B = 3, M = 14: boxes exactly on the matched and on the unmatched threshold, rows of the
classes 2 and 4 that no anchor class takes, class-0 rows with a real footprint, boxes off the grid, an interior zero row
and trailing zero rows.  Stored: the anchors per class and flattened, the boxes and the three outputs."""
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
                 'pcdet.ops.iou3d_nms.iou3d_nms_utils'):
        load(name)
    coder = load('pcdet.utils.box_coder_utils')
    gen = load('pcdet.models.dense_heads.target_assigner.anchor_generator')
    return coder, gen, load('pcdet.models.dense_heads.target_assigner.axis_aligned_target_assigner')


def main():
    coder, gen, assigner = load_reference()
    torch.set_num_threads(1)
    cfg = to_cfg(R.G27_HEAD_CFG)
    generator = gen.AnchorGenerator(anchor_range=R.G27_RANGE, anchor_generator_config=cfg.ANCHOR_GENERATOR_CONFIG)
    grid = np.array(R.G27_GRID)
    anchors, per_loc = generator.generate_anchors([grid[:2] // c['feature_map_stride'] for c in cfg.ANCHOR_GENERATOR_CONFIG])
    assert per_loc == [3, 6, 3] and all(tuple(a.shape[:3]) == (1, 17, 17) for a in anchors)
    target = assigner.AxisAlignedTargetAssigner(model_cfg=cfg, class_names=R.G27_CLASS_NAMES, box_coder=coder.ResidualCoder(),
                                                match_height=False)
    gt = R.g27_boxes()
    d = target.assign_targets(anchors, torch.from_numpy(gt.copy()))
    out = {'gt_boxes': gt}
    for k, a in enumerate(anchors):
        out['anchors%d' % k] = _np(a)
    out['anchors'] = _np(torch.cat(anchors, dim=-3).view(-1, 7))
    out['box_cls_labels'], out['box_reg_targets'] = _np(d['box_cls_labels']), _np(d['box_reg_targets'])
    out['reg_weights'] = _np(d['reg_weights'])
    lab = out['box_cls_labels']
    assert lab.dtype == np.int32 and lab.shape == (R.G27_B, 17 * 17 * 12) and set(np.unique(lab)) == {-1, 0, 1, 3, 5}
    meta = {'torch': torch.__version__, 'seed': R.G27_SEED, 'num_anchors_per_location': per_loc, 'classes': R.G27_CLASS_NAMES,
            'anchor_classes': [c['class_name'] for c in R.G27_ANCHOR_CFG]}
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'g27_anchor_assigner.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'positives per sample:', (lab > 0).sum(1).tolist(), 'ignored:', (lab == -1).sum(1).tolist())


if __name__ == '__main__':
    main()
