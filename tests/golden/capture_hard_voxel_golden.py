"""Golden G23: the reference's own MeanVFE (row f-19 of SURVEY.md section 8) on voxels made by the restatement of
csrc/dfu3d_hvox.h (tests/hard_voxel_ref.py).

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_hard_voxel_golden.py REFERENCE_ROOT      ->  tests/golden/g23_hard_voxel.npz

pcdet/models/backbones_3d/vfe/mean_vfe.py is imported UNMODIFIED as a member of a package skeleton; its base class
`vfe_template.VFETemplate` is a stand-in (an nn.Module that keeps model_cfg: MeanVFE uses nothing else of it).

The scene: 400 rows of four columns in a 6 x 5 x 2 grid, T = 5, at most 40 voxels; among the voxels one that is full, one
whose single row is (x, y, z, -0.0), and, appended behind the restatement's, one with 0 points (all slots +0.0): the
reference divides it by clamp_min(0, 1).

Stored: points, point_cnt, range_min, voxel_size, grid, max_points, max_voxels (the restatement's inputs), voxels,
voxel_num_points (MeanVFE's inputs) and voxel_features (its output).
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from tests import hard_voxel_ref as H  # noqa: E402

RMIN, VS, GRID, T, MAX_VOXELS = (0.0, -2.5, -1.0), (0.5, 1.0, 1.5), (6, 5, 2), 5, 40


def load_reference():
    for name in ('pcdet', 'pcdet.models', 'pcdet.models.backbones_3d', 'pcdet.models.backbones_3d.vfe'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    tmpl = types.ModuleType('pcdet.models.backbones_3d.vfe.vfe_template')

    class VFETemplate(torch.nn.Module):
        def __init__(self, model_cfg, **kwargs):
            super().__init__()
            self.model_cfg = model_cfg
    tmpl.VFETemplate = VFETemplate
    sys.modules[tmpl.__name__] = tmpl
    name = 'pcdet.models.backbones_3d.vfe.mean_vfe'
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, 'pcdet/models/backbones_3d/vfe/mean_vfe.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def scene():
    rng = np.random.default_rng(23)
    n = 400
    cell = np.stack([rng.integers(0, 6, n), rng.integers(0, 5, n), rng.integers(0, 2, n)], 1).astype(np.float64)
    cell[7] = (5, 4, 1)                                          # the only row of its cell, with a -0.0 feature
    cell[(cell == (5, 4, 1)).all(1) & (np.arange(n) != 7)] = (0, 0, 0)
    xyz = np.asarray(RMIN) + (cell + rng.uniform(0.1, 0.9, cell.shape)) * np.asarray(VS)
    pts = np.concatenate([np.zeros((n, 1)), xyz, rng.uniform(-3, 3, (n, 1))], 1).astype(np.float32)
    pts[7, 4] = -0.0
    return pts, np.array([n], np.int32)


def main():
    mod = load_reference()
    vfe = mod.MeanVFE(model_cfg={}, num_point_features=4)
    pts, cnt = scene()
    out = H.hard_voxels(pts, cnt, RMIN, VS, GRID, T, MAX_VOXELS)
    nv = int(out['n_voxels'][0])
    voxels = np.concatenate([out['voxels'][:nv], np.zeros((1, T, 4), np.float32)])
    num = np.concatenate([out['voxel_num_points'][:nv], np.zeros(1, np.int32)])
    v7 = int(out['point_voxel'][7])
    assert num.max() == T and num[v7] == 1 and np.signbit(voxels[v7, 0, 3]) and num[-1] == 0 and nv == MAX_VOXELS
    got = vfe.forward({'voxels': torch.from_numpy(voxels), 'voxel_num_points': torch.from_numpy(num)})
    feats = got['voxel_features'].numpy()
    assert feats.shape == (nv + 1, 4) and feats.dtype == np.float32 and vfe.get_output_feature_dim() == 4
    path = os.path.join(HERE, 'g23_hard_voxel.npz')
    np.savez_compressed(path, points=pts, point_cnt=cnt, range_min=np.array(RMIN, np.float32),
                        voxel_size=np.array(VS, np.float32), grid=np.array(GRID, np.int32), max_points=np.int64(T),
                        max_voxels=np.int64(MAX_VOXELS), voxels=voxels, voxel_num_points=num, voxel_features=feats)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
