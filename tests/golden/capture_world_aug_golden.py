"""Golden G15: the reference's own world augmentation, range masks and collate (row f-10 of SURVEY.md section 8) over ten
synthetic scenes under two configurations.

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_world_aug_golden.py REFERENCE_ROOT      ->  tests/golden/g15_world_aug.npz

pcdet/datasets/augmentor/data_augmentor.py, augmentor_utils.py, pcdet/utils/common_utils.py, box_utils.py,
pcdet/datasets/processor/data_processor.py, point_feature_encoder.py and pcdet/datasets/dataset.py are imported UNMODIFIED
as members of a package skeleton.  Import-time stand-ins, all empty: `SharedArray`, `skimage`, `torchvision`, the compiled
ops and `database_sampler` (no configuration here has a gt_sampling entry).

Configuration 0 has the CenterPoint YAML's shape: float32 boxes of 7 columns, flip along x, rotation, scaling,
translation, training (boxes masked), a range with a zero bound.  Configuration 1: float64 boxes of 9 columns, flips
along x and y, a scale range narrower than 1e-3 (no draw), training=False (boxes not masked; the augmentor is run by this
script, since dataset.py runs it in training only).  Both have names outside class_names.

The reference's random_world_scaling cannot return from a narrow range (global_scaling gives two values there, three
are unpacked): the queue entries are wrapped by a recorder, which also turns that ValueError into "nothing drawn,
nothing changed" -- global_scaling returns before it touches anything.

Scenes 0..7: 0, 1, 63, 64, 1023, 1024, 1025, 3000 points and 0, 1, 40, 64, 65, 200, 1, 40 boxes.  Scenes 8, 9 go through
an augmentor of the same configuration with rotation range [0, 0], no scaling and zero translation noise, and carry
planted points and box centres exactly on every face of the range, one float32 step inside and outside it, and -0.0.

Stored per scene: the inputs, the drawn values, the boxes after every step, the points' xyz after the rotation and
after the whole augmentor, the keys of the dicts, the final per-scene boxes and the point keep mask (the script asserts
that the final points ARE the augmented points under that mask), and per configuration the collated gt_boxes, the
batch-index column of the collated points (asserted to be the concatenation otherwise) and NumPy's final RNG state.
"""
import importlib.util
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from tests import world_aug_ref as R  # noqa: E402

CLASSES = ['Car', 'Pedestrian', 'Cyclist']
NAMES = ['Car', 'Pedestrian', 'Cyclist', 'Truck', 'Van']
SEEDS = [151, 152]
N_POINTS = [0, 1, 63, 64, 1023, 1024, 1025, 3000]
N_BOXES = [0, 1, 40, 64, 65, 200, 1, 40]
RANGES = [[0.0, -39.68, -3.0, 69.12, 39.68, 1.0], [-51.2, -51.2, -5.0, 51.2, 51.2, 3.0]]
STEPS = ['random_world_flip', 'random_world_rotation', 'random_world_scaling', 'random_world_translation']


class Cfg(dict):
    __getattr__ = dict.__getitem__


def to_cfg(x):
    if isinstance(x, dict):
        return Cfg({k: to_cfg(v) for k, v in x.items()})
    return [to_cfg(v) for v in x] if isinstance(x, list) and x and isinstance(x[0], dict) else x


def load_reference():
    for name in ('pcdet', 'pcdet.ops', 'pcdet.ops.iou3d_nms', 'pcdet.ops.roiaware_pool3d', 'pcdet.utils',
                 'pcdet.datasets', 'pcdet.datasets.augmentor', 'pcdet.datasets.processor', 'skimage'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    for name in ('SharedArray', 'torchvision', 'skimage.transform', 'pcdet.ops.iou3d_nms.iou3d_nms_utils',
                 'pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils', 'pcdet.datasets.augmentor.database_sampler'):
        sys.modules[name] = types.ModuleType(name)
        if '.' in name:
            setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], sys.modules[name])

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)
        return mod
    load('pcdet.utils.common_utils', 'pcdet/utils/common_utils.py')
    load('pcdet.utils.box_utils', 'pcdet/utils/box_utils.py')
    load('pcdet.datasets.augmentor.augmentor_utils', 'pcdet/datasets/augmentor/augmentor_utils.py')
    aug = load('pcdet.datasets.augmentor.data_augmentor', 'pcdet/datasets/augmentor/data_augmentor.py')
    load('pcdet.datasets.processor.point_feature_encoder', 'pcdet/datasets/processor/point_feature_encoder.py')
    load('pcdet.datasets.processor.data_processor', 'pcdet/datasets/processor/data_processor.py')
    ds = load('pcdet.datasets.dataset', 'pcdet/datasets/dataset.py')
    return aug, ds


def aug_config(ci, planted):
    flip = {'NAME': 'random_world_flip', 'ALONG_AXIS_LIST': ['x'] if ci == 0 else ['x', 'y']}
    rot = {'NAME': 'random_world_rotation', 'WORLD_ROT_ANGLE': [0.0, 0.0] if planted else [-0.78539816, 0.78539816]}
    scale = {'NAME': 'random_world_scaling',
             'WORLD_SCALE_RANGE': [1.0, 1.0] if planted else ([0.95, 1.05] if ci == 0 else [1.0, 1.0005])}
    trans = {'NAME': 'random_world_translation',
             'NOISE_TRANSLATE_STD': [0.0, 0.0, 0.0] if planted else [0.5, 0.5, 0.5]}
    return {'DISABLE_AUG_LIST': ['placeholder'], 'AUG_CONFIG_LIST': [flip, rot, scale, trans]}


def dataset_config(ci, planted):
    return {
        'POINT_CLOUD_RANGE': RANGES[ci], 'DATA_PATH': '.',
        'POINT_FEATURE_ENCODING': {'encoding_type': 'absolute_coordinates_encoding',
                                   'used_feature_list': ['x', 'y', 'z', 'intensity'],
                                   'src_feature_list': ['x', 'y', 'z', 'intensity']},
        'DATA_AUGMENTOR': aug_config(ci, planted),
        'DATA_PROCESSOR': [{'NAME': 'mask_points_and_boxes_outside_range', 'REMOVE_OUTSIDE_BOXES': True},
                           {'NAME': 'transform_points_to_voxels_placeholder', 'VOXEL_SIZE': [0.2, 0.2, 8.0]}],
    }


def steps32(v):
    v = np.float32(v)
    return [np.nextafter(v, np.float32(-np.inf)), v, np.nextafter(v, np.float32(np.inf))]


def planted_scene(rng, ci, nbox_cols):
    r = np.array(RANGES[ci], np.float32)
    pts, ctr = [], []
    mid = (r[0:3] + r[3:6]) / np.float32(2)
    for axis in range(3):
        for bound in (r[axis], r[axis + 3]):
            for v in steps32(bound) + ([np.float32(-0.0)] if bound == 0 else []):
                q = mid.copy()
                q[axis] = v
                ctr.append(q)
                if axis < 2:
                    pts.append(q)
    for zv in (r[2] - 1, r[5] + 1):                    # no z test for points
        pts.append(np.array([mid[0], mid[1], zv], np.float32))
    pts = np.array(pts, np.float32)
    p = np.concatenate([pts, rng.integers(0, 256, (len(pts), 1)).astype(np.float32) / 256], 1).astype(np.float32)
    b = np.zeros((len(ctr), nbox_cols))
    b[:, 0:3] = np.array(ctr, np.float32)
    b[:, 3:6] = [3.9, 1.6, 1.5]
    b[:, 6] = rng.uniform(-7, 7, len(ctr))
    if nbox_cols > 7:
        b[:, 7:9] = rng.uniform(-5, 5, (len(ctr), 2))
    names = np.array([NAMES[k % 3] for k in range(len(ctr))])
    return p, b, names


def make_scenes(rng, ci):
    nb = 7 if ci == 0 else 9
    lo, hi = (np.array([-40.0, -60.0, -4.0]), np.array([90.0, 60.0, 2.0])) if ci == 0 else \
        (np.array([-80.0, -80.0, -6.0]), np.array([80.0, 80.0, 4.0]))
    scenes = []
    for n, m in zip(N_POINTS, N_BOXES):
        p = np.zeros((n, 4), np.float32)
        p[:, 0:3] = np.round(rng.uniform(lo, hi, (n, 3)) * 64) / 64          # coarse inputs: they compress
        p[:, 3] = rng.integers(0, 256, n) / 256
        b = np.zeros((m, nb))
        r = np.array(RANGES[ci])
        ext = 0.15 * (r[3:6] - r[0:3])                                       # boxes: the range and 15 % around it
        b[:, 0:3] = rng.uniform(r[0:3] - ext, r[3:6] + ext, (m, 3))
        b[:, 3:6] = rng.uniform(0.5, 5.0, (m, 3))
        b[:, 6] = rng.uniform(-10.0, 10.0, m)                                 # beyond one period: the wrap works
        if nb > 7:
            b[:, 7:9] = rng.uniform(-8, 8, (m, 2))
        names = np.array([NAMES[int(k)] for k in rng.integers(0, len(NAMES), m)], dtype='<U10')
        scenes.append((p, b, names, False))
    for _ in range(2):
        scenes.append(planted_scene(rng, ci, nb) + (True,))
    return scenes


def main():
    aug_mod, ds_mod = load_reference()

    class Dataset(ds_mod.DatasetTemplate):
        def __len__(self):
            return 1

        def __getitem__(self, index):                 # prepare_data's resample of a scene that kept no box
            return {'resampled': True}

    rng = np.random.default_rng(2015)
    out = {'class_names': np.array(CLASSES), 'numpy_version': np.array(np.__version__), 'n_scenes': np.array(10),
           'steps': np.array(STEPS)}
    for ci in range(2):
        training = ci == 0
        dt = np.float32 if ci == 0 else np.float64
        out['range/%d' % ci] = np.array(RANGES[ci], np.float32)
        out['training/%d' % ci] = np.array(training)
        recorded = {}

        def wrap(augmentor):
            for k, entry in enumerate(list(augmentor.data_augmentor_queue)):
                def run(data_dict=None, entry=entry, k=k):
                    try:
                        data_dict = entry(data_dict=data_dict)
                    except ValueError:
                        cfg = entry.keywords['config']
                        assert cfg['NAME'] == 'random_world_scaling' and \
                            cfg['WORLD_SCALE_RANGE'][1] - cfg['WORLD_SCALE_RANGE'][0] < 1e-3
                    recorded[STEPS[k]] = (data_dict['points'].copy(), data_dict['gt_boxes'].copy())
                    return data_dict
                augmentor.data_augmentor_queue[k] = run

        sets = {}
        for planted in (False, True):
            cfg = to_cfg(dataset_config(ci, planted))
            out['cfg/%d/%d' % (ci, int(planted))] = np.array(json.dumps(dataset_config(ci, planted)))
            d = Dataset(dataset_cfg=cfg, class_names=CLASSES, training=training, root_path='.')
            a = d.data_augmentor if training else aug_mod.DataAugmentor('.', cfg.DATA_AUGMENTOR, CLASSES)
            assert len(a.data_augmentor_queue) == 4
            wrap(a)
            after = {}
            fwd = a.forward

            def rec_fwd(data_dict, fwd=fwd, after=after):
                r = fwd(data_dict)
                after['dict'] = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in r.items()}
                return r
            a.forward = rec_fwd
            final = {}
            proc = d.data_processor.forward

            def rec_proc(data_dict, proc=proc, final=final):
                r = proc(data_dict=data_dict)
                final['dict'] = dict(r)
                final['rng'] = np.random.get_state()
                return r
            d.data_processor.forward = rec_proc
            sets[planted] = (d, a, after, final)
        scenes = make_scenes(rng, ci)
        np.random.seed(SEEDS[ci])
        finals = []
        for s, (p, b, names, planted) in enumerate(scenes):
            d, a, after, final = sets[planted]
            b = b.astype(dt)
            pre = '%d/%d/' % (ci, s)
            out['in/' + pre + 'points'], out['in/' + pre + 'gt_boxes'], out['in/' + pre + 'gt_names'] = p, b, names
            out['planted/' + pre[:-1]] = np.array(planted)
            dd = {'points': p.copy(), 'gt_boxes': b.copy(), 'gt_names': names.copy()}
            recorded.clear()
            if training:
                d.prepare_data(dd)
                np.random.set_state(final['rng'])      # the resample's randint is dataset business, not this row's
            else:
                mask = np.array([n in CLASSES for n in names], dtype=np.bool_)
                d.prepare_data(a.forward({**dd, 'gt_boxes_mask': mask}))
            A, F = after['dict'], final['dict']
            for k, name in enumerate(STEPS):
                out['step/' + pre + name + '/gt_boxes'] = recorded[name][1]
            out['step/' + pre + 'random_world_rotation/xyz'] = recorded['random_world_rotation'][0][:, 0:3]
            assert np.array_equal(recorded['random_world_translation'][0], A['points'])
            assert np.array_equal(A['points'][:, 3], p[:, 3])
            out['aug/' + pre + 'xyz'] = A['points'][:, 0:3]
            out['aug/' + pre + 'gt_boxes'], out['aug/' + pre + 'gt_names'] = A['gt_boxes'], A['gt_names']
            out['aug/' + pre + 'keys'] = np.array(sorted(A.keys()))
            for axis in ('x', 'y'):
                if 'flip_' + axis in A:
                    out['drawn/' + pre + 'flip_' + axis] = np.array(A['flip_' + axis])
            out['drawn/' + pre + 'noise_rot'] = np.array(A['noise_rot'])
            out['drawn/' + pre + 'noise_scale'] = np.array(A.get('noise_scale', np.nan))
            out['drawn/' + pre + 'noise_translate'] = A['noise_translate']
            keep = R.point_mask(A['points'], RANGES[ci])
            assert np.array_equal(A['points'][keep].view(np.int32), F['points'].view(np.int32))
            out['final/' + pre + 'point_keep'] = keep
            out['final/' + pre + 'gt_boxes'] = F['gt_boxes']
            out['final/' + pre + 'keys'] = np.array(sorted(k for k in F.keys() if k != 'gt_names'))
            finals.append({'points': F['points'], 'gt_boxes': F['gt_boxes']})
            # (a) neither a pass-through nor a drop-all can pass
            if len(p) >= 1023:
                assert 0.2 <= 1 - keep.mean() <= 0.8, (ci, s, keep.mean())
            if len(b) >= 40:
                assert len(F['gt_boxes']) >= 2 and len(b) - len(F['gt_boxes']) >= 2, (ci, s, len(F['gt_boxes']))
            # (b) the planted scenes are not rotated, scaled or moved
            if planted:
                assert A['noise_rot'] == 0.0 and 'noise_scale' not in A and not A['noise_translate'].any()
            # (c) the restatement reproduces every point scene of 64 rows or more bit for bit
            drawn = {'flips': [(ax, bool(A['flip_' + ax])) for ax in a_axes(ci)], 'noise_rot': A['noise_rot'],
                     'noise_scale': A.get('noise_scale'), 'noise_translate': A['noise_translate']}
            rp, _, _ = R.augment(p, b, drawn)
            if len(p) >= 64:
                assert np.array_equal(rp.view(np.int32), A['points'].view(np.int32)), (ci, s)
        batch = Dataset.collate_batch(finals)
        cat = np.concatenate([f['points'] for f in finals], 0)
        assert np.array_equal(batch['points'][:, 1:].view(np.int32), cat.view(np.int32))
        out['batch/%d/batch_index' % ci] = batch['points'][:, 0].astype(np.int8)
        out['batch/%d/gt_boxes' % ci] = batch['gt_boxes']
        st = np.random.get_state()
        out['rng/%d/keys' % ci] = st[1]
        out['rng/%d/pos' % ci] = np.array(st[2])
    path = os.path.join(HERE, 'g15_world_aug.npz')
    np.savez_compressed(path, **out)
    print('wrote %s: %.1f KB' % (path, os.path.getsize(path) / 1e3))


def a_axes(ci):
    return ['x'] if ci == 0 else ['x', 'y']


if __name__ == '__main__':
    main()
