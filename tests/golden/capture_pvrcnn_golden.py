"""Golden G26: the reference's own VoxelSetAbstraction, PointHeadSimple and PVRCNNHead, run on the CPU.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_pvrcnn_golden.py REFERENCE_ROOT      ->  tests/golden/g26_pvrcnn.npz

pcdet/models/backbones_3d/pfe/voxel_set_abstraction.py, pcdet/models/roi_heads/pvrcnn_head.py with
roi_head_template.py, pcdet/models/dense_heads/point_head_simple.py with point_head_template.py, and
pcdet/ops/pointnet2/pointnet2_stack/pointnet2_utils.py / pointnet2_modules.py are imported UNMODIFIED as members of a
package skeleton, with the reference's own utils they import.  Stand-ins, written below: a `pointnet2_stack_cuda` module
whose wrappers fill the output tensors from the sequential NumPy float32 restatements of tests/point_stack_ref.py,
empty compiled leaves (`roiaware_pool3d_cuda`, `iou3d_nms_cuda`: the RoIs are given, so no NMS runs), an empty
`SharedArray`, `Tensor.cuda` mapped to the identity and torch.cuda.IntTensor / FloatTensor to the CPU types.

As G19, G26 therefore pins the reference's own ORCHESTRATION -- which op feeds which, the sources' order in the
concatenation, the cycling of a short sample's keypoints, the bilinear arithmetic (torch on the CPU: the reference's own
code), the grid points, the wiring of the heads, the state-dict keys -- and NOT its kernels' arithmetic.

Fixture (tests/point_stack_ref.py: G26_*): B = 2 with 300 and 40 points (the second shorter than NUM_KEYPOINTS = 48), a
16 x 12 BEV map of 8 channels, four sparse levels made from the points' own voxels, GRID_SIZE 2 and 6 RoIs per sample,
seeded weights with BatchNorm statistics away from the default, eval mode.
"""
import copy
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

from tests import point_stack_ref as R  # noqa: E402

REC = {'ball': [], 'fps': []}


class Cfg(dict):
    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key)


def to_cfg(d):
    return Cfg({k: to_cfg(v) if isinstance(v, dict) else copy.deepcopy(v) for k, v in d.items()})


def _np(t):
    return t.detach().numpy()


# ---- the stand-in of pointnet2_stack_cuda ------------------------------------------------------------------------------
def ball_query_wrapper(B, M, radius, nsample, new_xyz, new_xyz_batch_cnt, xyz, xyz_batch_cnt, idx):
    out, empty = R.ball_query(_np(xyz), R.starts(_np(xyz_batch_cnt)), _np(new_xyz), R.starts(_np(new_xyz_batch_cnt)),
                              radius, nsample)
    REC['ball'].append((out.copy(), empty.copy()))
    marked = out.copy()
    marked[empty == 1, 0] = -1                         # the kernel's mark of an empty ball; the wrapper cleans it up
    idx.copy_(torch.from_numpy(marked))


def group_points_wrapper(B, M, C, nsample, features, features_batch_cnt, idx, idx_batch_cnt, output):
    f, i = _np(features), _np(idx)
    zeros = np.zeros((len(f), 3), np.float32)
    out = R.group(zeros, R.starts(_np(features_batch_cnt)), np.zeros((M, 3), np.float32), R.starts(_np(idx_batch_cnt)),
                  f, i, np.zeros(M, np.uint8))
    output.copy_(torch.from_numpy(np.ascontiguousarray(out[3:].transpose(1, 0, 2))))


def farthest_point_sampling_wrapper(B, N, npoint, xyz, temp, output):
    out = np.zeros((B, npoint), np.int32)
    for b in range(B):
        picks = R.fps_one(_np(xyz)[b], min(N, npoint))  # beyond N picks the caller overwrites the rest
        out[b, :len(picks)] = picks
    REC['fps'].append(out.copy())
    output.copy_(torch.from_numpy(out))


def load_reference():
    names = ('pcdet', 'pcdet.ops', 'pcdet.ops.pointnet2', 'pcdet.ops.pointnet2.pointnet2_stack', 'pcdet.ops.roiaware_pool3d',
             'pcdet.ops.iou3d_nms', 'pcdet.utils', 'pcdet.models', 'pcdet.models.backbones_3d',
             'pcdet.models.backbones_3d.pfe', 'pcdet.models.dense_heads', 'pcdet.models.roi_heads',
             'pcdet.models.roi_heads.target_assigner', 'pcdet.models.model_utils')
    for name in names:
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        if '.' in name:
            setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)
    sys.modules['SharedArray'] = types.ModuleType('SharedArray')
    for name, fns in (('pcdet.ops.pointnet2.pointnet2_stack.pointnet2_stack_cuda',
                       {'ball_query_wrapper': ball_query_wrapper, 'group_points_wrapper': group_points_wrapper,
                        'farthest_point_sampling_wrapper': farthest_point_sampling_wrapper}),
                      ('pcdet.ops.roiaware_pool3d.roiaware_pool3d_cuda', {}), ('pcdet.ops.iou3d_nms.iou3d_nms_cuda', {})):
        m = types.ModuleType(name)
        m.__dict__.update(fns)
        sys.modules[name] = m
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)
    torch.cuda.IntTensor, torch.cuda.FloatTensor = torch.IntTensor, torch.FloatTensor
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
                 'pcdet.models.model_utils.model_nms_utils', 'pcdet.models.roi_heads.target_assigner.proposal_target_layer',
                 'pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils', 'pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules',
                 'pcdet.models.dense_heads.point_head_template', 'pcdet.models.roi_heads.roi_head_template'):
        load(name)
    return (load('pcdet.models.backbones_3d.pfe.voxel_set_abstraction'), load('pcdet.models.dense_heads.point_head_simple'),
            load('pcdet.models.roi_heads.pvrcnn_head'))


def make_fixture(rng):
    """points (340, 5) in the range, their voxels at the four strides as sparse levels, a BEV map, RoIs."""
    lo, hi = np.asarray(R.G26_RANGE[:3]), np.asarray(R.G26_RANGE[3:])
    pts = []
    for b, n in enumerate(R.G26_COUNTS):
        centres = rng.uniform(lo + 0.8, hi - 0.8, (5, 3))
        xyz = centres[rng.integers(5, size=n)] + rng.normal(0.0, 0.35, (n, 3))
        xyz = np.clip(xyz, lo + 0.01, hi - 0.01)
        pts.append(np.concatenate([np.full((n, 1), b), xyz, rng.uniform(0.0, 1.0, (n, 1))], axis=1))
    pts = np.concatenate(pts).astype(np.float32)
    out = {'points': pts}
    cell = np.floor((pts[:, 1:4] - lo.astype(np.float32)) / np.asarray(R.G26_VOXEL, np.float32)).astype(np.int64)
    for name, cfg in R.G26_PFE['SA_LAYER'].items():
        if name == 'raw_points':
            continue
        f = cfg['DOWNSAMPLE_FACTOR']
        keys = np.unique(np.concatenate([pts[:, :1].astype(np.int64), (cell // f)[:, ::-1]], axis=1), axis=0)   # b, z, y, x
        out[name + '_indices'] = keys.astype(np.int32)
        out[name + '_features'] = rng.normal(0.0, 1.0, (len(keys), R.G26_LEVEL_CHANNELS[name])).astype(np.float32)
    out['spatial_features'] = rng.normal(0.0, 1.0, (R.G26_B,) + R.G26_BEV).astype(np.float32)
    rois = np.zeros((R.G26_B, R.G26_ROIS, 7), np.float32)
    for b in range(R.G26_B):
        own = pts[pts[:, 0] == b, 1:4]
        rois[b, :, 0:3] = own[rng.integers(len(own), size=R.G26_ROIS)] + rng.normal(0.0, 0.2, (R.G26_ROIS, 3))
        rois[b, :, 3:6] = rng.uniform([1.2, 0.6, 0.6], [2.4, 1.2, 1.2], (R.G26_ROIS, 3))
        rois[b, :, 6] = rng.uniform(-np.pi, np.pi, R.G26_ROIS)
    rois[1, -1, 0:3] += 30.0                            # an RoI far from every keypoint: empty balls
    out['rois'] = rois
    return out


def randomise_norms(model, rng):
    for m in model.modules():
        if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)):
            m.running_mean.copy_(torch.from_numpy(rng.normal(0, 0.3, m.num_features).astype(np.float32)))
            m.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
            m.weight.data.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
            m.bias.data.copy_(torch.from_numpy(rng.normal(0, 0.2, m.num_features).astype(np.float32)))


class Level:
    def __init__(self, indices, features):
        self.indices, self.features = indices, features


def main():
    vsa_mod, ph_mod, rh_mod = load_reference()
    rng = np.random.default_rng(2600)
    torch.manual_seed(2600)
    torch.set_num_threads(1)
    out, meta = {}, {'torch': torch.__version__}
    pfe = vsa_mod.VoxelSetAbstraction(to_cfg(R.G26_PFE), R.G26_VOXEL, R.G26_RANGE, num_bev_features=R.G26_BEV[0],
                                      num_rawpoint_features=4)
    point_head = ph_mod.PointHeadSimple(num_class=1, input_channels=pfe.num_point_features_before_fusion,
                                        model_cfg=to_cfg(R.G26_POINT_HEAD))
    roi_head = rh_mod.PVRCNNHead(input_channels=pfe.num_point_features, model_cfg=to_cfg(R.G26_ROI_HEAD), num_class=1)
    with torch.no_grad():
        roi_head.reg_layers[-1].weight.mul_(300.0)      # (init: normal(0, 0.001): residuals that move the boxes)
    for tag, model in (('pfe', pfe), ('point_head', point_head), ('roi_head', roi_head)):
        randomise_norms(model, rng)
        model.eval()
        sd = model.state_dict()
        meta[tag + '_keys'] = list(sd)
        for k, v in sd.items():
            out['sd_%s_%s' % (tag, k)] = v.numpy().copy()
    fix = make_fixture(rng)
    out.update(fix)
    batch = dict(batch_size=R.G26_B, points=torch.from_numpy(fix['points'].copy()),
                 spatial_features=torch.from_numpy(fix['spatial_features'].copy()),
                 spatial_features_stride=R.G26_BEV_STRIDE,
                 multi_scale_3d_features={n: Level(torch.from_numpy(fix[n + '_indices'].copy()),
                                                   torch.from_numpy(fix[n + '_features'].copy()))
                                          for n in R.G26_LEVEL_CHANNELS},
                 rois=torch.from_numpy(fix['rois'].copy()), roi_scores=torch.zeros(R.G26_B, R.G26_ROIS),
                 roi_labels=torch.ones(R.G26_B, R.G26_ROIS, dtype=torch.long), has_class_labels=False)
    with torch.no_grad():
        batch = pfe(batch)
        out['bev_features'] = _np(pfe.interpolate_from_bev_features(
            batch['point_coords'], batch['spatial_features'], R.G26_B, bev_stride=R.G26_BEV_STRIDE)).copy()
        n_pfe_balls = len(REC['ball'])
        batch = point_head(batch)
        glob, local = roi_head.get_global_grid_points_of_roi(batch['rois'], grid_size=R.G26_ROI_HEAD['ROI_GRID_POOL']['GRID_SIZE'])
        out['global_grid_points'], out['local_grid_points'] = _np(glob).copy(), _np(local).copy()
        before = len(REC['ball'])
        out['pooled_features'] = _np(roi_head.roi_grid_pool(batch)).copy()
        del REC['ball'][before:]                        # the forward below queries the same balls again
        batch = roi_head(batch)
    sources = ['raw_points'] + [n for n in R.G26_PFE['FEATURES_SOURCE'] if n not in ('bev', 'raw_points')]
    assert n_pfe_balls == 2 * len(sources) and len(REC['ball']) == n_pfe_balls + 2 and len(REC['fps']) == R.G26_B
    for k, src in enumerate(sources + ['roi_grid']):     # the reference's call order: raw points first
        for s in range(2):
            idx, empty = REC['ball'][2 * k + s]
            out['ball_%s_%d' % (src, s)], out['empty_%s_%d' % (src, s)] = idx, empty
            print(src, s, 'empty balls %d of %d' % (empty.sum(), len(empty)),
                  'distinct indices per ball: mean %.2f' % np.mean([len(set(r)) for r in idx]))
    for key in ('point_coords', 'point_features_before_fusion', 'point_features', 'point_cls_scores', 'batch_cls_preds',
                'batch_box_preds'):
        out[key] = _np(batch[key]).copy()
    assert out['empty_roi_grid_0'].any() and (out['point_coords'][48:, 0] == 1).all()
    assert np.array_equal(out['point_coords'][88:96], out['point_coords'][48:56])      # the short sample's picks again
    meta['largest'] = {k: float(np.abs(out[k]).max()) for k in ('point_features', 'pooled_features', 'batch_box_preds')}
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'g26_pvrcnn.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), meta['torch'], meta['largest'])


if __name__ == '__main__':
    main()
