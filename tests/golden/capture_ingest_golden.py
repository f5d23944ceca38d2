"""Golden G18: the reference's own KittiDataset over three synthetic frames (row f-13 of SURVEY.md section 8).

Run in the build container (needs the reference tree; nothing at test time does):
    python tests/golden/capture_ingest_golden.py REFERENCE_ROOT      ->  tests/golden/g18_ingest.npz

pcdet/datasets/kitti/kitti_dataset.py, pcdet/utils/box_utils.py, calibration_kitti.py, object3d_kitti.py and
common_utils.py are imported UNMODIFIED by file path as members of a package skeleton.  Import-time stand-ins:
`SharedArray`, `pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils` and `pcdet.datasets.kitti.kitti_utils` are empty;
`skimage.io` is absent on the capture machine and gets an `imread` over PIL (get_image_shape reads nothing but `.shape`);
`pcdet.datasets.dataset.DatasetTemplate` pulls in the augmentor, the processor and the compiled ops, so it is a stand-in
that only stores the constructor's arguments (root_path as a Path, `mode` from `training`).

Captured, all from the reference's code running unmodified over a KITTI directory written from the frames of
tests/ingest_cases.py golden_specs(): `KittiDataset.get_infos(count_inside_pts=True)` (every annotation key, with
`gt_boxes_lidar` and the `in_hull` counts `num_points_in_gt`), `KittiDataset.get_fov_flag` over `lidar_to_rect` as
`__getitem__` calls it, and `box_utils.boxes3d_kitti_camera_to_lidar` over the DontCare-free camera boxes as `__getitem__`
builds them (common_utils.drop_info_with_name).  NOT captured, because DatasetTemplate is a stand-in: `__getitem__` itself
(prepare_data) and `__len__`; their class selection is checked against tests/ingest_ref.py and select_classes alone.

The script asserts that no point of a frame lies within 1e-4 m of a face plane of one of its boxes -- in fact none within
1 mm of a z face or 2 cm of an x / y face, which covers the 1 cm margin of csrc/pt_in_box.hpp -- and that the hull counts
equal the counts of tests/ingest_ref.py on these frames."""
import importlib.util
import os
import sys
import tempfile
import types
from pathlib import Path

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('PCDET_REFERENCE', '')

from tests import ingest_cases as K  # noqa: E402
from tests import ingest_ref as R  # noqa: E402


class Cfg(dict):
    __getattr__ = dict.__getitem__


class DatasetTemplate(object):
    def __init__(self, dataset_cfg=None, class_names=None, training=True, root_path=None, logger=None):
        self.dataset_cfg, self.class_names, self.training, self.logger = dataset_cfg, class_names, training, logger
        self.root_path = Path(root_path)
        self.mode = 'train' if training else 'test'
        self._merge_all_iters_to_one_epoch = False


def load_reference():
    for name in ('pcdet', 'pcdet.ops', 'pcdet.ops.roiaware_pool3d', 'pcdet.utils', 'pcdet.datasets', 'pcdet.datasets.kitti',
                 'skimage'):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
    for name in ('SharedArray', 'skimage.io', 'pcdet.ops.roiaware_pool3d.roiaware_pool3d_utils',
                 'pcdet.datasets.kitti.kitti_utils', 'pcdet.datasets.dataset'):
        sys.modules[name] = types.ModuleType(name)
        if '.' in name:
            setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], sys.modules[name])
    from PIL import Image
    sys.modules['skimage.io'].imread = lambda path: np.array(Image.open(str(path)))
    sys.modules['pcdet.datasets.dataset'].DatasetTemplate = DatasetTemplate

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        setattr(sys.modules[name.rsplit('.', 1)[0]], name.rsplit('.', 1)[1], mod)
        return mod
    common = load('pcdet.utils.common_utils', 'pcdet/utils/common_utils.py')
    box = load('pcdet.utils.box_utils', 'pcdet/utils/box_utils.py')
    load('pcdet.utils.calibration_kitti', 'pcdet/utils/calibration_kitti.py')
    load('pcdet.utils.object3d_kitti', 'pcdet/utils/object3d_kitti.py')
    ds = load('pcdet.datasets.kitti.kitti_dataset', 'pcdet/datasets/kitti/kitti_dataset.py')
    return common, box, ds


def main():
    if not REF:
        sys.exit("usage: capture_ingest_golden.py REFERENCE_ROOT")
    common, box_utils, ds = load_reference()
    frames = [K.make_frame(**s) for s in K.golden_specs()]
    out = {'n_frames': np.array(len(frames))}
    with tempfile.TemporaryDirectory() as root:
        K.write_kitti(root, frames, split='train')
        cfg = Cfg(DATA_SPLIT={'train': 'train', 'test': 'train'}, INFO_PATH={'train': [], 'test': []}, FOV_POINTS_ONLY=True)
        dataset = ds.KittiDataset(dataset_cfg=cfg, class_names=K.CLASSES, training=False, root_path=root)
        assert dataset.sample_id_list == [f['id'] for f in frames]
        infos = dataset.get_infos(num_workers=1, has_label=True, count_inside_pts=True)
        for i, (f, info) in enumerate(zip(frames, infos)):
            p = 'f%d_' % i
            assert info['point_cloud'] == {'num_features': 4, 'lidar_idx': f['id']}
            for k in ('id', 'label'):
                out[p + k] = np.frombuffer(f[k].encode(), np.uint8)
            for k in ('points', 'P2', 'R0', 'V2C', 'shape'):
                out[p + k] = f[k]
            out[p + 'image_shape'] = info['image']['image_shape']
            for k in ('P2', 'R0_rect', 'Tr_velo_to_cam'):
                out[p + 'calib_' + k] = info['calib'][k]
            ann = info['annos']
            assert sorted(ann) == sorted(K.INFO_KEYS), sorted(ann)
            for k in K.INFO_KEYS:
                out[p + 'ann_' + k] = np.asarray(ann[k]) if k != 'name' else np.asarray(ann[k]).astype('U')
            calib = dataset.get_calib(f['id'])
            points = dataset.get_lidar(f['id'])
            assert np.array_equal(points.view(np.uint32), f['points'].view(np.uint32))
            flag = dataset.get_fov_flag(calib.lidar_to_rect(points[:, 0:3]), info['image']['image_shape'], calib)
            out[p + 'fov_flag'] = flag
            clean = common.drop_info_with_name(ann, name='DontCare')
            cam = np.concatenate([clean['location'], clean['dimensions'], clean['rotation_y'][..., np.newaxis]],
                                 axis=1).astype(np.float32)
            out[p + 'getitem_names'] = np.asarray(clean['name']).astype('U')
            out[p + 'boxes_camera'] = cam
            out[p + 'getitem_boxes'] = box_utils.boxes3d_kitti_camera_to_lidar(cam, calib) if len(cam) else np.zeros((0, 7))
            # the condition under which the hull and the box rule agree, and that they do
            boxes = ann['gt_boxes_lidar']
            if len(boxes):
                d = K.face_distance(points, boxes)
                assert d[..., 0].min() >= K.BAND_XY > 1e-2 + 1e-4 and d[..., 1].min() >= K.BAND_Z > 1e-4, d.min((0, 1))
            want = R.box_counts(points[flag], boxes)
            n_obj = len(boxes)
            assert np.array_equal(ann['num_points_in_gt'][:n_obj], want), (ann['num_points_in_gt'], want)
            assert (ann['num_points_in_gt'][n_obj:] == -1).all()
            assert np.array_equal(flag, R.fov_flag(points, K.calib_of(f), f['shape']))
            print(f['id'], 'points', len(points), 'kept', int(flag.sum()), 'num_points_in_gt', ann['num_points_in_gt'])
    np.savez_compressed(os.path.join(HERE, 'g18_ingest.npz'), **out)
    print('wrote g18_ingest.npz,', os.path.getsize(os.path.join(HERE, 'g18_ingest.npz')), 'bytes')


if __name__ == '__main__':
    main()
