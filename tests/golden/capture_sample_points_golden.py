"""Golden G22: the reference's own DataProcessor.sample_points (row f-18 of SURVEY.md section 8) on eight small scenes,
one per branch of the rule of csrc/dfu3d_smp.h, under four NumPy seeds each.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_sample_points_golden.py REFERENCE_ROOT      ->  tests/golden/g22_sample_points.npz

pcdet/datasets/processor/data_processor.py is imported UNMODIFIED as a member of a package skeleton; `skimage`,
`torchvision` and `pcdet.utils` are empty import-time stand-ins (sample_points uses none of them).  The method is
called on an object made without __init__ (which only builds the queue), with mode 'train'.

A scene is float32 (n, 4): x, y, z and the row's own index, which survives `points[choice]` and so records the choice.
Every scene with far rows carries the depth boundary: (40, 0, 0) and (24, 32, 0), whose depth is exactly 40 and not
near, and their float32 neighbours just below in x resp. y.

Stored per scene s: points_s, k_s (NUM_POINTS), rows_s int32 (seeds, k_s): the chosen row of every output row.  The script
asserts the contract of tests/sample_points_ref.py on every output and, in the scenes with fewer than k far rows, that
every near row (by the restatement's flags) is missing from the output of some seed: the witness that the reference
took it for near.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from tests import sample_points_ref as S  # noqa: E402

SEEDS = [221, 222, 223, 224]
# (n, K, F): F rows at or beyond 40 m (None: the depth is not looked at)
SCENES = [(96, 40, 35), (96, 4, 0), (96, 40, 40), (96, 40, 70), (40, 40, None), (30, 40, None), (20, 40, None),
          (7, 40, None)]


class Cfg(dict):
    __getattr__ = dict.__getitem__


def load_reference():
    for name in ('pcdet', 'pcdet.utils', 'pcdet.datasets', 'pcdet.datasets.processor', 'skimage'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    for name in ('torchvision', 'skimage.transform', 'pcdet.utils.box_utils', 'pcdet.utils.common_utils'):
        sys.modules[name] = types.ModuleType(name)
        if '.' in name:
            setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], sys.modules[name])
    name = 'pcdet.datasets.processor.data_processor'
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, 'pcdet/datasets/processor/data_processor.py'))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def below(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def scene(rng, n, far):
    """n rows; `far` of them (None: a third) at 41 .. 70 m, the rest within 39 m; with far rows, the boundary rows."""
    n_far = n // 3 if far is None else far
    is_far = np.zeros(n, bool)
    is_far[rng.permutation(n)[:n_far]] = True
    ang = rng.uniform(-np.pi, np.pi, n)
    rad = np.where(is_far, rng.uniform(41.0, 70.0, n), rng.uniform(2.0, 39.0, n))
    pts = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.5, 0.5, n) * 0.01], 1).astype(np.float32)
    if far:
        at_far, at_near = np.flatnonzero(is_far), np.flatnonzero(~is_far)
        pts[at_far[0]] = (40.0, 0.0, 0.0)
        pts[at_far[1]] = (24.0, 32.0, 0.0)
        if len(at_near) >= 2:
            pts[at_near[0]] = (below(40.0), 0.0, 0.0)
            pts[at_near[1]] = (24.0, below(below(below(32.0))), 0.0)
    pts = np.concatenate([pts, np.arange(n, dtype=np.float32)[:, None]], 1)
    if far is not None:
        assert int((~S.near_flags(pts[:, 0:3])).sum()) == far, (n, far)
    return pts


def main():
    mod = load_reference()
    dp = object.__new__(mod.DataProcessor)
    dp.mode = 'train'
    rng = np.random.default_rng(22)
    out = {'seeds': np.array(SEEDS, np.int64), 'n_scenes': np.int64(len(SCENES))}
    for s, (n, K, far) in enumerate(SCENES):
        pts = scene(rng, n, far)
        cfg = Cfg(NAME='sample_points', NUM_POINTS={'train': K, 'test': K})
        rows = []
        for seed in SEEDS:
            np.random.seed(seed)
            got = dp.sample_points(data_dict={'points': pts.copy()}, config=cfg)['points']
            assert got.shape == (K, 4)
            r = got[:, 3].astype(np.int32)
            assert np.array_equal(got, pts[r])
            S.check_contract(pts[:, 0:3], r, K)
            rows.append(r)
        rows = np.stack(rows)
        if far is not None and far < K:
            near = S.near_flags(pts[:, 0:3])
            seen_always = np.array([all(i in set(r.tolist()) for r in rows) for i in range(n)])
            assert not (seen_always & near).any(), "a near row is in every seed's output: no witness"
            assert seen_always[~near].all()
        out['points_%d' % s], out['k_%d' % s], out['rows_%d' % s] = pts, np.int64(K), rows
    path = os.path.join(HERE, 'g22_sample_points.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
