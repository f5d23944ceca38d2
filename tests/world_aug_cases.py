"""Golden G15 (tests/golden/g15_world_aug.npz, written by tests/golden/capture_world_aug_golden.py) read once and turned
into the operands the world-augmentation tests share: per scene the inputs and the drawn values, and the restatement's
results (tests/world_aug_ref.py), computed once per configuration and never modified."""
import functools
import json
import os

import numpy as np

from tests import world_aug_ref as R

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g15_world_aug.npz")
N_CFG = 2
EPS = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def n_scenes():
    return int(golden()['n_scenes'])


def class_names():
    return [str(c) for c in golden()['class_names']]


def axes(ci):
    return json.loads(str(golden()['cfg/%d/0' % ci]))['DATA_AUGMENTOR']['AUG_CONFIG_LIST'][0]['ALONG_AXIS_LIST']


def dataset_cfg(ci, planted):
    return json.loads(str(golden()['cfg/%d/%d' % (ci, int(planted))]))


def pc_range(ci):
    return golden()['range/%d' % ci]


def training(ci):
    return bool(golden()['training/%d' % ci])


def planted(ci, s):
    return bool(golden()['planted/%d/%d' % (ci, s)])


def inputs(ci, s):
    G = golden()
    pre = 'in/%d/%d/' % (ci, s)
    return G[pre + 'points'], G[pre + 'gt_boxes'], G[pre + 'gt_names']


def drawn(ci, s):
    G = golden()
    pre = 'drawn/%d/%d/' % (ci, s)
    sc = float(G[pre + 'noise_scale'])
    return {'flips': [(a, bool(G[pre + 'flip_' + a])) for a in axes(ci)], 'noise_rot': float(G[pre + 'noise_rot']),
            'noise_scale': None if np.isnan(sc) else sc, 'noise_translate': G[pre + 'noise_translate']}


@functools.lru_cache(maxsize=None)
def restated(ci):
    """-> (per scene [(points, gt_boxes, keep rows, augmented points, augmented boxes, steps)], batch of all scenes)."""
    per, ops = [], []
    for s in range(n_scenes()):
        p, b, names = inputs(ci, s)
        cls = R.class_ids(names, class_names())
        d = drawn(ci, s)
        ap, ab, steps = R.augment(p, b, d)
        fp, fg, keep = R.scene(p, b, cls, d, pc_range(ci), mask_boxes=training(ci))
        per.append((fp, fg, keep, ap, ab, steps))
        ops.append((p, b, cls, d))
    return per, R.batch(ops, pc_range(ci), mask_boxes=training(ci))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


def rot_bound(x, y):
    """The bound of the numerics contract for a rotated coordinate of a list under 64 rows: one rounding of a product
    plus one of the sum, 2^-23 (|x| + |y|), x and y the coordinates that went into the rotation."""
    return EPS * (np.abs(x) + np.abs(y))
