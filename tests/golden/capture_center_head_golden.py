"""Golden G12: the reference's own CenterHead geometry (row f-6 of SURVEY.md section 8) -- `CenterHead.assign_targets`
and `centernet_utils.decode_bbox_from_heatmap`, run unmodified on the CPU.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_center_head_golden.py REFERENCE_ROOT      ->  tests/golden/g12_center_head.npz

pcdet/models/model_utils/centernet_utils.py and pcdet/models/dense_heads/center_head.py are imported UNMODIFIED as members
of a package skeleton.  Import-time stand-ins: `numba` (its `jit` returns the function; circle_nms is never called),
`model_nms_utils` and `loss_utils` (empty, unused on this path).  `assign_targets` is called on an object made with
object.__new__(CenterHead) that carries only model_cfg, class_names, class_names_each_head, point_cloud_range
(a float32 array, as the dataset makes it) and voxel_size (the config's list).  The (centre cell, radius) of every drawn
Gaussian is recorded by wrapping `draw_gaussian_to_heatmap`.

Configuration A: the CenterPoint config of the labels (10 classes, 6 heads, stride 4, 128 x 64 map, NUM_MAX_OBJS 500,
C = 8).  Configuration B: 3 classes in 2 heads, stride 8, C = 10 (velocity), NUM_MAX_OBJS 8.  For each the script
asserts that every head run alone on a fresh copy of gt_boxes equals the joint run (the reference rewrites the class
column in place; G12 holds only cases where the two readings agree), and records the exception of a batch with
NUM_MAX_OBJS + 1 boxes of one head.  Heat maps are stored sparsely (flat index + value).
Decode: heat maps with provably distinct scores and random regression maps (tests/center_head_ref.py: decode_inputs;
their float64 sums are stored as a check), three cases.
"""
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

from tests.center_head_ref import CFG_A, CFG_B, decode_inputs  # noqa: E402

DECODE_CASES = [
    dict(seed=121, B=2, n_cls=2, K=500, vel=False, iou=False, score_thresh=0.98),
    dict(seed=122, B=2, n_cls=2, K=500, vel=True, iou=True, score_thresh=None),
    dict(seed=123, B=2, n_cls=1, K=700, vel=True, iou=False, score_thresh=0.93),
]
DECODE_LIMIT = [5.0, -45.0, -10.0, 45.0, 45.0, 10.0]


class Cfg(dict):
    __getattr__ = dict.__getitem__


def load_reference():
    for name in ('pcdet', 'pcdet.models', 'pcdet.models.model_utils', 'pcdet.models.dense_heads', 'pcdet.utils'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    numba = types.ModuleType('numba')
    numba.jit = lambda *a, **k: (lambda fn: fn)
    sys.modules['numba'] = numba
    for name in ('pcdet.models.model_utils.model_nms_utils', 'pcdet.utils.loss_utils'):
        m = types.ModuleType(name)
        sys.modules[name] = m
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], m)

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)
        return mod
    cu = load('pcdet.models.model_utils.centernet_utils', os.path.join(REF, 'pcdet/models/model_utils/centernet_utils.py'))
    ch = load('pcdet.models.dense_heads.center_head', os.path.join(REF, 'pcdet/models/dense_heads/center_head.py'))
    return cu, ch


def make_head(ch, cfg, heads=None):
    head = object.__new__(ch.CenterHead)
    head.model_cfg = Cfg(TARGET_ASSIGNER_CONFIG=Cfg(FEATURE_MAP_STRIDE=cfg['stride'], NUM_MAX_OBJS=cfg['num_max_objs'],
                                                    GAUSSIAN_OVERLAP=cfg['gaussian_overlap'], MIN_RADIUS=cfg['min_radius']))
    head.class_names = cfg['class_names']
    head.class_names_each_head = [list(h) for h in (heads if heads is not None else cfg['heads'])]
    head.point_cloud_range = np.array(cfg['point_cloud_range'], dtype=np.float32)
    head.voxel_size = cfg['voxel_size']
    return head


def box(rng, cfg, cls, x=None, y=None, size=None, scale=1.0):
    r = cfg['point_cloud_range']
    x = rng.uniform(r[0], r[3]) if x is None else x
    y = rng.uniform(r[1], r[4]) if y is None else y
    l, w, h = size if size is not None else (rng.uniform(0.4, 9.0) * scale, rng.uniform(0.4, 3.0) * scale, rng.uniform(0.8, 3.5))
    row = [x, y, rng.uniform(r[2], r[5]), l, w, h, rng.uniform(-np.pi, np.pi)]
    if cfg['C'] == 10:
        row += [rng.uniform(-8, 8), rng.uniform(-8, 8)]
    return row + [cls]


def scenes(cfg, rng):
    """The assign batch of a configuration and a one-sample batch with NUM_MAX_OBJS + 1 boxes of head 0."""
    r, C, nmax, n_cls = cfg['point_cloud_range'], cfg['C'], cfg['num_max_objs'], len(cfg['class_names'])
    out = []
    out.append([])                                                             # 0: no boxes
    s = []                                                                     # 1: zero-padded rows between real ones
    for k in range(30 if nmax >= 30 else 6):
        s.append(box(rng, cfg, 1 + int(rng.integers(n_cls))))
        if k % 3 == 0:
            s.append([0.0] * C)
    out.append(s)
    s = []                                                                     # 2: outside the range on every side, dx = 0
    for x, y in ((r[0] - 7, 0.0), (r[3] + 7, 3.0), (20.0, r[1] - 9), (25.0, r[4] + 9), (r[0] - 3, r[1] - 3),
                 (r[3] + 3, r[4] + 3), (r[0] - 1, r[4] + 2), (r[3] + 2, r[1] - 2), (r[0] + 0.3, 1.0), (r[3] - 0.05, r[4] - 0.05)):
        s.append(box(rng, cfg, 1 + len(s) % n_cls, x=x, y=y, size=(rng.uniform(4, 12), rng.uniform(2, 4), 2.0)))
    z = box(rng, cfg, 1, x=10.0, y=0.0)
    z[3] = 0.0
    s.insert(3, z)
    z = box(rng, cfg, n_cls, x=12.0, y=5.0)
    z[4] = 0.0
    s.append(z)
    out.append(s)
    s = []                                                                     # 3: same-class Gaussians that overlap
    for k in range(6):
        s.append(box(rng, cfg, 1, x=20.0 + 1.1 * k, y=-3.0 + 0.7 * k, size=(4.5 + k, 1.9, 1.6)))
    for k in range(2 if nmax < 30 else 8):
        s.append(box(rng, cfg, n_cls, x=30.0 + 0.5 * k, y=10.0, size=(0.6, 0.6, 1.7)))
    out.append(s)
    s = [box(rng, cfg, 1) for _ in range(nmax)]                                # 4: exactly NUM_MAX_OBJS boxes of head 0
    s += [box(rng, cfg, n_cls) for _ in range(3)]
    order = rng.permutation(len(s))
    out.append([s[i] for i in order])
    over = [box(rng, cfg, 1) for _ in range(nmax + 1)]
    M = max(len(s) for s in out) + 2
    gt = np.zeros((len(out), M, C), np.float32)
    for b, s in enumerate(out):
        if s:
            gt[b, :len(s)] = np.asarray(s, np.float32)
    return gt, np.asarray(over, np.float32)[None]


def main():
    cu, ch = load_reference()
    draws = []
    real_draw = cu.draw_gaussian_to_heatmap

    def recording_draw(heatmap, center, radius, k=1, valid_mask=None):
        draws.append((int(center[0]), int(center[1]), int(radius)))
        return real_draw(heatmap, center, radius, k=k, valid_mask=valid_mask)
    cu.draw_gaussian_to_heatmap = recording_draw

    out, meta = {}, {'decode_cases': DECODE_CASES, 'decode_limit': DECODE_LIMIT, 'torch': torch.__version__}
    for name, cfg, seed in (('A', CFG_A, 1201), ('B', CFG_B, 1202)):
        rng = np.random.default_rng(seed)
        gt, over = scenes(cfg, rng)
        H, W = cfg['map_hw']
        draws.clear()
        joint = make_head(ch, cfg).assign_targets(torch.from_numpy(gt.copy()), feature_map_size=[H, W])
        joint_draws = list(draws)
        assert joint['heatmap_masks'] == []
        pos = 0
        for h, names in enumerate(cfg['heads']):
            alone = make_head(ch, cfg, heads=[names]).assign_targets(torch.from_numpy(gt.copy()), feature_map_size=[H, W])
            for key in ('heatmaps', 'target_boxes', 'inds', 'masks', 'target_boxes_src'):
                assert torch.equal(alone[key][0], joint[key][h]), (name, h, key)
            hm = joint['heatmaps'][h].numpy()
            assert hm.shape == (gt.shape[0], len(names), H, W) and hm.dtype == np.float32
            idx = np.flatnonzero(hm)
            out['%s_h%d_hm_idx' % (name, h)] = idx.astype(np.int32)
            out['%s_h%d_hm_val' % (name, h)] = hm.reshape(-1)[idx]
            out['%s_h%d_target_boxes' % (name, h)] = joint['target_boxes'][h].numpy()
            out['%s_h%d_inds' % (name, h)] = joint['inds'][h].numpy()
            out['%s_h%d_masks' % (name, h)] = joint['masks'][h].numpy()
            out['%s_h%d_target_boxes_src' % (name, h)] = joint['target_boxes_src'][h].numpy()
            n = int(joint['masks'][h].sum())                      # the draws of head h, sample by sample, in slot order
            per = joint['masks'][h].sum(1).tolist()
            rows = [(b,) + d for b, cnt in enumerate(per) for d in joint_draws[pos + sum(per[:b]):pos + sum(per[:b]) + cnt]]
            out['%s_h%d_draws' % (name, h)] = np.asarray(rows, np.int32).reshape(-1, 4)
            pos += n
        assert pos == len(joint_draws)
        out[name + '_gt_boxes'] = gt
        out[name + '_over_gt_boxes'] = over
        try:
            make_head(ch, cfg).assign_targets(torch.from_numpy(over.copy()), feature_map_size=[H, W])
            meta[name + '_over_exception'] = None
        except Exception as e:                                    # noqa: BLE001 -- the recorded behaviour
            meta[name + '_over_exception'] = type(e).__name__
        exact = over[:, :cfg['num_max_objs']].copy()
        make_head(ch, cfg).assign_targets(torch.from_numpy(exact), feature_map_size=[H, W])   # no exception at the cap
    # decode
    H, W = CFG_A['map_hw']
    for i, case in enumerate(DECODE_CASES):
        d = decode_inputs(case['seed'], case['B'], case['n_cls'], H, W, case['vel'], case['iou'])
        t = {k: (None if v is None else torch.from_numpy(v)) for k, v in d.items()}
        res = cu.decode_bbox_from_heatmap(
            heatmap=t['heatmap'], rot_cos=t['rot_cos'], rot_sin=t['rot_sin'], center=t['center'], center_z=t['center_z'],
            dim=t['dim'], vel=t['vel'], iou=t['iou'], point_cloud_range=np.array(CFG_A['point_cloud_range'], np.float32),
            voxel_size=CFG_A['voxel_size'], feature_map_stride=CFG_A['stride'], K=case['K'], circle_nms=False,
            score_thresh=case['score_thresh'], post_center_limit_range=torch.tensor(DECODE_LIMIT).float())
        out['D%d_input_sums' % i] = np.asarray([v.astype(np.float64).sum() for v in d.values() if v is not None])
        for b, r in enumerate(res):
            assert 0 < len(r['pred_scores']) < case['K']
            for key, v in r.items():
                out['D%d_s%d_%s' % (i, b, key)] = v.numpy()
    out['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    path = os.path.join(HERE, 'g12_center_head.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), meta)


if __name__ == '__main__':
    main()
