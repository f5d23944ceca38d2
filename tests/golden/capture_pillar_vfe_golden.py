"""Golden G13: the reference's own dynamic pillar feature encoder, run on the CPU.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_pillar_vfe_golden.py REFERENCE_ROOT      ->  tests/golden/g13_pillar_vfe.npz

pcdet/models/backbones_3d/vfe/vfe_template.py and dynamic_pillar_vfe.py are imported UNMODIFIED as members of a package
skeleton.  Stand-ins: a `torch_scatter` module written below -- scatter_mean as index_add_ on the CPU (sequential in
the index order) divided by the count, scatter_max by scatter_reduce('amax') with the first index among equal maxima
as its argument -- and torch.Tensor.cuda as the identity.

G13 therefore pins the reference's own ORCHESTRATION: the mask, the key, the order of the sorted unique, the order of
the feature columns, the wiring of the layers and the coordinate columns.  It does NOT pin third-party arithmetic:
torch_scatter's float atomics have no defined order, and Linear / BatchNorm1d are torch's on whatever device runs them.

Configurations (tests/pillar_vfe_ref.py): A the CenterPoint config of the labels (range [0,-51.2,-5,51.2,51.2,3], voxel
[0.2,0.2,8], USE_ABSLOTE_XYZ, norm, filters [64,64], 4 raw features, batch 3 with sample 1 empty); B WITH_DISTANCE, no
absolute xyz, no norm, filters [32], grid 37 x 53; C DynamicPillarVFESimple2D.  Stored per configuration: the points,
the seeded state dict (BatchNorm statistics included) and its key list, unq_inv, unq_cnt, the coordinates, the matrix
entering the first PFN layer, every layer's post-ReLU x and its x_max (eval mode), the final features in eval() and in
train() mode; and the torch version.
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

from tests.pillar_vfe_ref import CFGS  # noqa: E402

N_POINTS = {'A': 360, 'B': 300, 'C': 260}
RECORD = []


class Cfg(dict):
    def __getattr__(self, key):
        try:
            return self[key]
        except KeyError:
            raise AttributeError(key)


def scatter_mean(src, index, dim=0):
    assert dim == 0 and src.device.type == 'cpu'
    n = int(index.max()) + 1 if index.numel() else 0
    out = torch.zeros((n,) + tuple(src.shape[1:]), dtype=src.dtype)
    out.index_add_(0, index, src)
    cnt = torch.bincount(index, minlength=n).clamp(min=1).to(src.dtype)
    return out / cnt.view(-1, *([1] * (src.dim() - 1)))


def scatter_max(src, index, dim=0):
    assert dim == 0 and src.dim() == 2
    n = int(index.max()) + 1 if index.numel() else 0
    idx = index.view(-1, 1).expand_as(src)
    out = torch.zeros((n, src.shape[1]), dtype=src.dtype).scatter_reduce(0, idx, src, 'amax', include_self=False)
    rows = torch.arange(src.shape[0]).view(-1, 1).expand_as(src)
    rows = torch.where(src == out[index], rows, torch.full_like(rows, src.shape[0]))
    arg = torch.full((n, src.shape[1]), src.shape[0], dtype=torch.int64).scatter_reduce(0, idx, rows, 'amin', include_self=True)
    RECORD.append((index.detach().numpy().copy(), src.detach().numpy().copy(), out.detach().numpy().copy()))
    return out, arg


def load_reference():
    for name in ('pcdet', 'pcdet.models', 'pcdet.models.backbones_3d', 'pcdet.models.backbones_3d.vfe'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    ts = types.ModuleType('torch_scatter')
    ts.scatter_mean, ts.scatter_max = scatter_mean, scatter_max
    sys.modules['torch_scatter'] = ts
    torch.Tensor.cuda = lambda self, *a, **k: self

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)
        return mod
    base = os.path.join(REF, 'pcdet/models/backbones_3d/vfe')
    load('pcdet.models.backbones_3d.vfe.vfe_template', os.path.join(base, 'vfe_template.py'))
    return load('pcdet.models.backbones_3d.vfe.dynamic_pillar_vfe', os.path.join(base, 'dynamic_pillar_vfe.py'))


def make_points(cfg, rng, n):
    """Clusters a few cells wide (several points per pillar, several pillars per cluster), points outside the range on
    every side, points on the range's edges; sample 1 of configuration A stays empty."""
    r, F = cfg['point_cloud_range'], cfg['num_point_features']
    k = max(n // 20, 4)
    cx, cy = rng.uniform(r[0], r[3], k), rng.uniform(r[1], r[4], k)
    which = rng.integers(k, size=n)
    pts = np.zeros((n, 1 + F), np.float32)
    pts[:, 1] = cx[which] + rng.normal(0, 0.12, n)
    pts[:, 2] = cy[which] + rng.normal(0, 0.12, n)
    pts[:, 3] = rng.uniform(r[2], r[5], n)
    pts[:, 4:] = rng.uniform(0, 1, (n, F - 3))
    batches = [0, 2] if cfg['batch_size'] == 3 else list(range(cfg['batch_size']))
    pts[:, 0] = np.asarray(batches)[rng.integers(len(batches), size=n)]
    pts[:8, 1] = [r[0] - 0.5, r[3] + 0.5, r[0], r[3], r[0] + 1.0, r[0] + 1.0, r[0] + 1.0, r[0] + 1.0]
    pts[:8, 2] = [0.0, 0.0, r[1], 0.0, r[1] - 0.5, r[4] + 0.5, r[4], r[1]]
    return pts


def main():
    mod = load_reference()
    out, meta = {}, {'torch': torch.__version__, 'configs': sorted(CFGS)}
    for name, cfg in sorted(CFGS.items()):
        rng = np.random.default_rng(1300 + ord(name))
        torch.manual_seed(1300 + ord(name))
        vfe = getattr(mod, cfg['cls'])(model_cfg=Cfg(cfg['model_cfg']), num_point_features=cfg['num_point_features'],
                                       voxel_size=cfg['voxel_size'], grid_size=np.asarray(cfg['grid_size']),
                                       point_cloud_range=cfg['point_cloud_range'])
        for m in vfe.modules():                                   # BatchNorm statistics and affine away from the default
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(torch.from_numpy(rng.normal(0, 0.3, m.num_features).astype(np.float32)))
                m.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
                m.weight.data.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
                m.bias.data.copy_(torch.from_numpy(rng.normal(0, 0.2, m.num_features).astype(np.float32)))
        pts = make_points(cfg, rng, N_POINTS[name])
        sd = vfe.state_dict()
        meta[name + '_state_dict_keys'] = list(sd)
        for k, v in sd.items():
            out['%s_sd_%s' % (name, k)] = v.numpy().copy()
        first_in = []
        hook = vfe.pfn_layers[0].register_forward_pre_hook(lambda m, a: first_in.append(a[0].detach().numpy().copy()))
        vfe.eval()
        RECORD.clear()
        with torch.no_grad():
            res = vfe(dict(points=torch.from_numpy(pts.copy()), batch_size=cfg['batch_size']))
        hook.remove()
        assert len(RECORD) == len(cfg['model_cfg']['NUM_FILTERS']) and len(first_in) == 1
        inv = RECORD[0][0]
        out[name + '_points'] = pts
        out[name + '_unq_inv'] = inv.astype(np.int32)
        out[name + '_unq_cnt'] = np.bincount(inv).astype(np.int32)
        coords_key = 'voxel_coords' if 'voxel_coords' in res else 'pillar_coords'
        meta[name + '_coords_key'] = coords_key
        meta[name + '_out_keys'] = sorted(k for k in res if k not in ('points', 'batch_size'))
        out[name + '_coords'] = res[coords_key].numpy().astype(np.int32)
        out[name + '_features_in'] = first_in[0]
        for i, (idx, x, x_max) in enumerate(RECORD):
            assert np.array_equal(idx, inv)
            out['%s_l%d_x' % (name, i)] = x
            out['%s_l%d_x_max' % (name, i)] = x_max
        out[name + '_final_eval'] = res['pillar_features'].numpy().copy()
        tr = copy.deepcopy(vfe).train()
        with torch.no_grad():
            out[name + '_final_train'] = tr(dict(points=torch.from_numpy(pts.copy()),
                                                 batch_size=cfg['batch_size']))['pillar_features'].numpy().copy()
        print(name, 'points', len(pts), 'kept', len(inv), 'pillars', int(inv.max()) + 1, 'max count', int(np.bincount(inv).max()))
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'g13_pillar_vfe.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), meta['torch'])


if __name__ == '__main__':
    main()
