"""Golden G16: the reference's own PointPillarScatter / PointPillarScatter3d, BaseBEVBackbone and the convolutional part
of CenterHead (row f-11 of SURVEY.md section 8), run unmodified on the CPU.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_centerpoint_golden.py REFERENCE_ROOT      ->  tests/golden/g16_centerpoint.npz

pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py, pcdet/models/backbones_2d/base_bev_backbone.py and
pcdet/models/dense_heads/center_head.py are imported UNMODIFIED as members of a package skeleton.  Stand-ins:
`np.int = int` (the backbone's stride branch), a no-op `Tensor.cuda` (the head's constructor), empty
`model_nms_utils` / `centernet_utils` modules and a `loss_utils` whose two loss classes are empty modules (no parameters
there either).

(a) tests/centerpoint_cases.py SCATTER_CASES: features, coords, the canvas stored sparsely (every word that is not +0.0)
    with its shape; for GRAD_CASE the gradient of pillar_features under a random canvas gradient (stored by its seed).
(b) SMALL_MODEL's backbone and head: seeded weights (the state dicts), one input, the eval() outputs at one thread;
    the largest deviation of a second run at 16 threads is printed and stored in the meta record.
(c) the ordered state-dict keys and shapes of the full centerpoint_nuscenes2kitti.yaml model: global_step, the
    pfn_layers keys by the convention of golden G13, then the reference's own backbone and head.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from tests import centerpoint_cases as K  # noqa: E402
from tests import pillar_scatter_ref as R  # noqa: E402


def load_reference():
    for name in ('pcdet', 'pcdet.models', 'pcdet.models.model_utils', 'pcdet.models.dense_heads', 'pcdet.utils',
                 'pcdet.models.backbones_2d', 'pcdet.models.backbones_2d.map_to_bev'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    for name in ('pcdet.models.model_utils.model_nms_utils', 'pcdet.models.model_utils.centernet_utils',
                 'pcdet.utils.loss_utils'):
        m = types.ModuleType(name)
        sys.modules[name] = m
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)
    lu = sys.modules['pcdet.utils.loss_utils']
    lu.FocalLossCenterNet = type('FocalLossCenterNet', (nn.Module,), {})
    lu.RegLossCenterNet = type('RegLossCenterNet', (nn.Module,), {})
    np.int = int
    torch.Tensor.cuda = lambda self, *a, **k: self

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod
    return (load('pcdet.models.backbones_2d.map_to_bev.pointpillar_scatter',
                 'pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py'),
            load('pcdet.models.backbones_2d.base_bev_backbone', 'pcdet/models/backbones_2d/base_bev_backbone.py'),
            load('pcdet.models.dense_heads.center_head', 'pcdet/models/dense_heads/center_head.py'))


def make_head(ch, model, dataset, input_channels):
    return ch.CenterHead(model_cfg=K.cfg(model['DENSE_HEAD']), input_channels=input_channels,
                         num_class=len(dataset['class_names']), class_names=dataset['class_names'],
                         grid_size=np.array(dataset['grid_size']), point_cloud_range=np.array(dataset['point_cloud_range']),
                         voxel_size=dataset['voxel_size'], predict_boxes_when_training=False)


def small_outputs(bb, head, x, threads):
    torch.set_num_threads(threads)
    with torch.no_grad():
        d = bb({'spatial_features': x})
        y = head.shared_conv(d['spatial_features_2d'])
        preds = [h(y) for h in head.heads_list]
    out = {'spatial_features_2d': d['spatial_features_2d'].numpy().copy()}
    for i, p in enumerate(preds):
        for k, v in p.items():
            out['head%d_%s' % (i, k)] = v.numpy().copy()
    return out


def main():
    sc, bev, ch = load_reference()
    out, meta = {}, {'torch': torch.__version__}
    # (a)
    for name, cls, B, C, grid, P, seed in K.SCATTER_CASES:
        nx, ny, nz = grid
        f, coords = K.scatter_inputs(B, C, grid, P, seed, empty=(1,) if name == 's0' else (),
                                     corners=(0, 2) if name == 's0' else ())
        cfg = K.cfg({'NUM_BEV_FEATURES': C * nz, 'INPUT_SHAPE': list(grid)})
        mod = getattr(sc, cls)(cfg, grid_size=np.array(grid))
        ft = torch.from_numpy(f.copy()).requires_grad_(True)
        # the reference finds the batch size from the largest batch index: the last sample of every case is occupied
        assert coords[:, 0].max() == B - 1
        d = mod({'pillar_features': ft, 'voxel_coords': torch.from_numpy(coords.copy())})
        canvas = d['spatial_features'].detach().numpy()
        assert canvas.shape == (B, C * nz, ny, nx)
        idx, val, shape = R.sparse(canvas)
        out[name + '_features'], out[name + '_coords'] = f, coords
        out[name + '_canvas_idx'], out[name + '_canvas_val'], out[name + '_canvas_shape'] = idx.astype(np.int32), val, shape
        if name == K.GRAD_CASE:
            g = np.random.default_rng(seed + 1000).standard_normal(canvas.shape).astype(np.float32)
            d['spatial_features'].backward(torch.from_numpy(g))
            out[name + '_grad_features'] = ft.grad.numpy().copy()
            meta['grad_seed'] = seed + 1000
    # (b)
    torch.manual_seed(1600)
    small = K.SMALL_MODEL
    bb = bev.BaseBEVBackbone(K.cfg(small['BACKBONE_2D']), input_channels=K.SMALL_INPUT[1])
    head = make_head(ch, small, K.SMALL_DATASET, bb.num_bev_features)
    for m in list(bb.modules()) + list(head.modules()):                 # running statistics that are not the identity
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.2)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.2)
    bb.eval()
    head.eval()
    x = torch.randn(K.SMALL_INPUT)
    one = small_outputs(bb, head, x, 1)
    many = small_outputs(bb, head, x, 16)
    dev = max(float(np.abs(one[k].astype(np.float64) - many[k]).max()) for k in one)
    meta['thread_deviation'] = dev
    print('largest deviation between 1 and 16 threads:', dev)
    out['small_input'] = x.numpy()
    for k, v in one.items():
        out['small_out_' + k] = v
    for pre, mod in (('bb', bb), ('head', head)):
        sd = mod.state_dict()
        meta['small_%s_keys' % pre] = list(sd)
        for k, v in sd.items():
            out['small_%s_sd_%s' % (pre, k)] = v.numpy().copy()
    # (c)
    full = K.FULL_MODEL
    keys = [('global_step', [1])]
    widths = [K.FULL_DATASET['num_point_features'] + 6] + full['VFE']['NUM_FILTERS']
    for i in range(len(widths) - 1):
        last = i >= len(widths) - 2
        n_out = widths[i + 1] if last else widths[i + 1] // 2
        n_in = widths[i] if i == 0 else widths[i]
        pre = 'vfe.pfn_layers.%d.' % i
        keys += [(pre + 'linear.weight', [n_out, n_in]), (pre + 'norm.weight', [n_out]), (pre + 'norm.bias', [n_out]),
                 (pre + 'norm.running_mean', [n_out]), (pre + 'norm.running_var', [n_out]),
                 (pre + 'norm.num_batches_tracked', [])]
    fbb = bev.BaseBEVBackbone(K.cfg(full['BACKBONE_2D']), input_channels=full['MAP_TO_BEV']['NUM_BEV_FEATURES'])
    fhead = make_head(ch, full, K.FULL_DATASET, fbb.num_bev_features)
    keys += [('backbone_2d.' + k, list(v.shape)) for k, v in fbb.state_dict().items()]
    keys += [('dense_head.' + k, list(v.shape)) for k, v in fhead.state_dict().items()]
    meta['full_keys'] = [k for k, _ in keys]
    meta['full_shapes'] = [s for _, s in keys]
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez_compressed(K.PATH, **out)
    print(K.PATH, os.path.getsize(K.PATH), len(keys), 'keys')


if __name__ == '__main__':
    main()
