"""Golden G19: the reference's own PointNet2MSG backbone, run on the CPU.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_pointnet2_golden.py REFERENCE_ROOT      ->  tests/golden/g19_pointnet2.npz

pcdet/ops/pointnet2/pointnet2_batch/pointnet2_utils.py, pointnet2_modules.py and
pcdet/models/backbones_3d/pointnet2_backbone.py are imported UNMODIFIED as members of a package skeleton.  Stand-ins,
written below: a `pointnet2_batch_cuda` module whose wrappers fill the output tensors from the sequential NumPy float32
restatements of tests/pointnet2_ref.py, empty pointnet2_stack modules (the backbone file imports them, PointNet2MSG does
not use them), and torch.cuda.IntTensor / FloatTensor mapped to the CPU types.

As G13, G19 therefore pins the reference's own ORCHESTRATION -- which op feeds which, the order of the channels and of
the concatenations, the weights of the interpolation, the wiring of the levels, the state-dict keys -- and NOT its
kernels' arithmetic: the CUDA kernels' tie rule in farthest point sampling depends on the block size and their backward
is a float atomicAdd.  The coordinates are drawn from a continuous distribution and the script checks that no sampling
step has two candidates of equal running minimum, so the tie rule plays no part in the stored indices.

Small model (tests/pointnet2_ref.py: G19_CFG): B = 2, N = 256, one extra feature, seeded state dict with BatchNorm
statistics away from the default, eval mode.  Stored: the points, the state dict and its key list, per SA level the FPS
indices, new_xyz and every scale's ball indices, per FP level the three-NN indices and distances, point_features and
point_coords (one thread; the largest deviation of a second run at 16 threads is stored in the meta record), the key list
of the full pointrcnn_nuscenes2kitti.yaml backbone, and the torch version.
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

from tests import pointnet2_ref as R  # noqa: E402

RECORD = {'fps': [], 'new_xyz': [], 'ball': [], 'nn': []}
TIES = []


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


def fps_wrapper(B, N, npoint, xyz, temp, output):
    idx, _ = R.fps(_np(xyz), npoint, ties=TIES)
    output.copy_(torch.from_numpy(idx))
    RECORD['fps'].append(idx.copy())


def gather_wrapper(B, C, N, npoint, features, idx, output):
    out = R.group(None, None, _np(features), _np(idx)[:, :, None], use_xyz=False)[..., 0]
    output.copy_(torch.from_numpy(out))
    if C == 3:
        RECORD['new_xyz'].append(out.transpose(0, 2, 1).copy())


def ball_wrapper(B, N, npoint, radius, nsample, new_xyz, xyz, idx):
    out = R.ball_query(_np(xyz), _np(new_xyz), radius, nsample)
    idx.copy_(torch.from_numpy(out))
    RECORD['ball'].append(out.copy())


def group_wrapper(B, C, N, npoint, nsample, features, idx, output):
    output.copy_(torch.from_numpy(R.group(None, None, _np(features), _np(idx), use_xyz=False)))


def three_nn_wrapper(B, n, m, unknown, known, dist2, idx):
    d2, i = R.three_nn_sq(_np(unknown), _np(known))
    dist2.copy_(torch.from_numpy(d2))                   # the reference takes the root of this
    idx.copy_(torch.from_numpy(i))
    RECORD['nn'].append((np.sqrt(d2), i.copy()))


def interpolate_wrapper(B, c, m, n, features, idx, weight, output):
    output.copy_(torch.from_numpy(R.three_interpolate(_np(features), _np(idx), _np(weight))))


def load_reference():
    names = ('pcdet', 'pcdet.ops', 'pcdet.ops.pointnet2', 'pcdet.ops.pointnet2.pointnet2_batch',
             'pcdet.ops.pointnet2.pointnet2_stack', 'pcdet.ops.pointnet2.pointnet2_stack.pointnet2_modules',
             'pcdet.ops.pointnet2.pointnet2_stack.pointnet2_utils', 'pcdet.models', 'pcdet.models.backbones_3d')
    for name in names:
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        if '.' in name:
            setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)
    cu = types.ModuleType('pcdet.ops.pointnet2.pointnet2_batch.pointnet2_batch_cuda')
    cu.farthest_point_sampling_wrapper, cu.gather_points_wrapper = fps_wrapper, gather_wrapper
    cu.ball_query_wrapper, cu.group_points_wrapper = ball_wrapper, group_wrapper
    cu.three_nn_wrapper, cu.three_interpolate_wrapper = three_nn_wrapper, interpolate_wrapper
    sys.modules[cu.__name__] = cu
    sys.modules['pcdet.ops.pointnet2.pointnet2_batch'].pointnet2_batch_cuda = cu
    torch.cuda.IntTensor, torch.cuda.FloatTensor = torch.IntTensor, torch.FloatTensor

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)
        return mod
    base = os.path.join(REF, 'pcdet/ops/pointnet2/pointnet2_batch')
    load('pcdet.ops.pointnet2.pointnet2_batch.pointnet2_utils', os.path.join(base, 'pointnet2_utils.py'))
    load('pcdet.ops.pointnet2.pointnet2_batch.pointnet2_modules', os.path.join(base, 'pointnet2_modules.py'))
    return load('pcdet.models.backbones_3d.pointnet2_backbone',
                os.path.join(REF, 'pcdet/models/backbones_3d/pointnet2_backbone.py'))


def make_points(rng):
    """Two samples of clustered points (a few hits per ball at the small radii, full balls at the large ones)."""
    B, N = R.G19_B, R.G19_N
    centres = rng.uniform(-3.0, 3.0, (B, 12, 3))
    which = rng.integers(12, size=(B, N))
    xyz = np.take_along_axis(centres, which[..., None].repeat(3, -1), axis=1) + rng.normal(0.0, 0.45, (B, N, 3))
    pts = np.zeros((B * N, 4 + R.G19_EXTRA), np.float32)
    pts[:, 0] = np.repeat(np.arange(B), N)
    pts[:, 1:4] = xyz.reshape(-1, 3)
    pts[:, 4:] = rng.uniform(0.0, 1.0, (B * N, R.G19_EXTRA))
    return pts


def run(model, pts, threads):
    torch.set_num_threads(threads)
    for v in RECORD.values():
        v.clear()
    with torch.no_grad():
        res = model(dict(points=torch.from_numpy(pts.copy()), batch_size=R.G19_B))
    return res['point_features'].numpy().copy(), res['point_coords'].numpy().copy()


def main():
    mod = load_reference()
    rng = np.random.default_rng(1900)
    torch.manual_seed(1900)
    out, meta = {}, {'torch': torch.__version__}
    meta['full_state_dict_keys'] = list(mod.PointNet2MSG(to_cfg(R.FULL_CFG), R.FULL_INPUT_CHANNELS).state_dict())
    model = mod.PointNet2MSG(to_cfg(R.G19_CFG), 3 + R.G19_EXTRA)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.running_mean.copy_(torch.from_numpy(rng.normal(0, 0.3, m.num_features).astype(np.float32)))
            m.running_var.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
            m.weight.data.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, m.num_features).astype(np.float32)))
            m.bias.data.copy_(torch.from_numpy(rng.normal(0, 0.2, m.num_features).astype(np.float32)))
    model.eval()
    sd = model.state_dict()
    meta['state_dict_keys'] = list(sd)
    for k, v in sd.items():
        out['sd_' + k] = v.numpy().copy()
    pts = make_points(rng)
    feats16, _ = run(model, pts, 16)
    feats, coords = run(model, pts, 1)
    assert not TIES, TIES                                 # no sampling step had two candidates at the maximum
    n_sa, n_fp = len(R.G19_CFG['SA_CONFIG']['NPOINTS']), len(R.G19_CFG['FP_MLPS'])
    assert len(RECORD['fps']) == len(RECORD['new_xyz']) == n_sa and len(RECORD['nn']) == n_fp
    assert len(RECORD['ball']) == sum(len(r) for r in R.G19_CFG['SA_CONFIG']['RADIUS'])
    out['points'] = pts
    balls = iter(RECORD['ball'])
    for k in range(n_sa):
        out['sa%d_fps_idx' % k] = RECORD['fps'][k]
        out['sa%d_new_xyz' % k] = RECORD['new_xyz'][k]
        for s in range(len(R.G19_CFG['SA_CONFIG']['RADIUS'][k])):
            b = next(balls)
            out['sa%d_ball%d' % (k, s)] = b
            print('SA', k, 'scale', s, 'distinct indices per ball: mean %.2f' % np.mean([len(set(r)) for r in b.reshape(-1, b.shape[-1])]))
    for j, (dist, idx) in enumerate(RECORD['nn']):        # in call order: the deepest FP level first
        level = n_fp - 1 - j
        out['fp%d_nn_dist' % level], out['fp%d_nn_idx' % level] = dist, idx
    out['point_features'], out['point_coords'] = feats, coords
    meta['thread_deviation'] = float(np.abs(feats16 - feats).max())
    print('largest deviation between 1 and 16 threads:', meta['thread_deviation'], 'largest |feature|:', float(np.abs(feats).max()))
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'g19_pointnet2.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), meta['torch'])


if __name__ == '__main__':
    main()
