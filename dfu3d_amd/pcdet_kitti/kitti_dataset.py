"""pcdet/datasets/kitti/kitti_dataset.py for the CenterPoint configuration of this project.

The two ends of the self-evolution loop's evaluation step, as functions (the class delegates to them):
  * generate_prediction_dicts (:339-419): detector output (LiDAR boxes, scores, labels) -> KITTI annotation dictionaries
    and, optionally, result files `<frame_id>.txt`;
  * evaluation (:421-431): annotation dictionaries -> the official AP report, computed on the GPU (eval.py of this
    package) where the reference needs numba-CUDA.
`KittiDataset` (:13-156, 434-501) turns a KITTI-format directory -- what this project's labeller writes -- into the
model's input; `get_infos` / `create_kitti_infos` (:158-282, 504-553) turn its label files into the info pickles the
dataset reads.  The hot path of both -- lidar_to_rect, rect_to_img, the FOV comparisons, the gather and the count of the
kept points inside every box -- is ingest_ops.fov_ingest (include/dfu3d_ingest.h), for a whole batch of frames at once.

`ds[i]` is the reference's per-frame dict, NumPy in and out, through fov_ingest with B = 1.  `ds.batches(batch_size, ...)`
is the batched form: per batch the B files are read, the raw points are uploaded once, ONE fov_ingest cuts them, and the
device result goes straight to data_augmentor.prepare_batch; what it yields is the model's batch_dict with `frame_id`,
`calib` and `image_shape` lists added.  One host read per batch on top of prepare_batch's: the B kept counts.

Divergences from the reference: `num_points_in_gt` counts by the box rule of
points_in_boxes_cpu, not by the Delaunay hull; `GET_ITEM_LIST` entries other than `points` raise NotImplementedError;
`create_kitti_infos` honours `save_path` and writes the info files (the reference's copy has a fixed path and the info
half commented out); the image shape comes from the PNG header (PIL) or, without the file, from the infos; `ds[i]` stops
after prepare_data's class selection (augmentation and range masks are prepare_batch's, for a batch); the batched form
does not shuffle the points of a frame (`shuffle_points`), as prepare_batch never did.
"""
import copy
import os
import pickle
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

from . import box_utils
from . import eval as kitti_eval
from .._lib import Dfu3dError
from ..calibration import Calibration
from ..labels import read_label_file
from .centerpoint import _get
from .gt_database import annotations_from_label

_ROW = '%s -1 -1 %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f %.4f'


def _to_numpy(t):
    return t.detach().cpu().numpy() if hasattr(t, 'detach') else np.asarray(t)


def _empty_prediction(n):
    return {'name': np.zeros(n), 'truncated': np.zeros(n), 'occluded': np.zeros(n), 'alpha': np.zeros(n),
            'bbox': np.zeros([n, 4]), 'dimensions': np.zeros([n, 3]), 'location': np.zeros([n, 3]),
            'rotation_y': np.zeros(n), 'score': np.zeros(n), 'boxes_lidar': np.zeros([n, 7])}


def generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None):
    """batch_dict: 'frame_id', 'calib', 'image_shape' per sample; pred_dicts: per sample 'pred_boxes' (N,7),
    'pred_scores' (N), 'pred_labels' (N, 1-based).  -> list of annotation dictionaries (+ 'frame_id', 'boxes_lidar')."""
    annos = []
    for index, box_dict in enumerate(pred_dicts):
        scores = _to_numpy(box_dict['pred_scores'])
        boxes = _to_numpy(box_dict['pred_boxes'])
        labels = _to_numpy(box_dict['pred_labels'])
        pred = _empty_prediction(scores.shape[0])
        if scores.shape[0] != 0:
            calib = batch_dict['calib'][index]
            image_shape = _to_numpy(batch_dict['image_shape'][index])
            cam = box_utils.boxes3d_lidar_to_kitti_camera(boxes, calib)
            pred['name'] = np.array(class_names)[labels - 1]
            pred['alpha'] = -np.arctan2(-boxes[:, 1], boxes[:, 0]) + cam[:, 6]
            pred['bbox'] = box_utils.boxes3d_kitti_camera_to_imageboxes(cam, calib, image_shape=image_shape)
            pred['dimensions'] = cam[:, 3:6]
            pred['location'] = cam[:, 0:3]
            pred['rotation_y'] = cam[:, 6]
            pred['score'] = scores
            pred['boxes_lidar'] = boxes
        pred['frame_id'] = batch_dict['frame_id'][index]
        annos.append(pred)
        if output_path is not None:
            with open(os.path.join(str(output_path), '%s.txt' % pred['frame_id']), 'w') as f:
                bbox, loc, dims = pred['bbox'], pred['location'], pred['dimensions']      # dims: l h w -> file: h w l
                for k in range(len(bbox)):
                    print(_ROW % (pred['name'][k], pred['alpha'][k], bbox[k][0], bbox[k][1], bbox[k][2], bbox[k][3],
                                  dims[k][1], dims[k][2], dims[k][0], loc[k][0], loc[k][1], loc[k][2],
                                  pred['rotation_y'][k], pred['score'][k]), file=f)
    return annos


def evaluation(det_annos, class_names, gt_annos):
    """kitti_dataset.py:421-431 with the ground-truth annotations handed in (the reference takes them from its info
    file) -> (report text, AP dictionary)."""
    if gt_annos is None:
        return None, {}
    return kitti_eval.get_official_eval_result(copy.deepcopy(list(gt_annos)), copy.deepcopy(list(det_annos)), class_names)


# ---- the dataset -----------------------------------------------------------------------------------------------------
ANNO_KEYS = ('name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score',
             'difficulty', 'index', 'gt_boxes_lidar')


def annotations_of(objs, calib):
    """kitti_dataset.py:184-260 for one frame: every key of the reference's `annos` but num_points_in_gt, in its order and
    its dtypes; an empty label file gives the reference's empty arrays."""
    objs = list(objs)
    a = annotations_from_label(objs, calib)
    n_obj = a['gt_boxes_lidar'].shape[0]
    if objs:
        more = {'truncated': np.array([o.truncation for o in objs]), 'occluded': np.array([o.occlusion for o in objs]),
                'alpha': np.array([o.alpha for o in objs]), 'dimensions': np.array([[o.l, o.h, o.w] for o in objs]),
                'location': np.concatenate([o.loc.reshape(1, 3) for o in objs], axis=0),
                'rotation_y': np.array([o.ry for o in objs]),
                'index': np.array(list(range(n_obj)) + [-1] * (len(objs) - n_obj), dtype=np.int32)}
    else:
        more = {'truncated': np.array([]), 'occluded': np.array([]), 'alpha': np.array([]), 'dimensions': np.zeros((0, 3)),
                'location': np.zeros((0, 3)), 'rotation_y': np.array([]), 'index': np.zeros((0,), dtype=np.int32)}
    a.update(more)
    return {k: a[k] for k in ANNO_KEYS}


def drop_info_with_name(info, name):
    """common_utils.drop_info_with_name: the rows of every array whose `name` is not `name`."""
    keep = [i for i, x in enumerate(info['name']) if x != name]
    return {k: v[keep] for k, v in info.items()}


class _Encoder:
    def __init__(self, num_point_features):
        self.num_point_features = num_point_features


class KittiDataset(object):
    """Drop-in for pcdet.datasets.kitti.kitti_dataset.KittiDataset in this configuration.  dataset_cfg: a dict or an
    attribute object with DATA_SPLIT, INFO_PATH, FOV_POINTS_ONLY and, for `batches`, POINT_CLOUD_RANGE, DATA_PROCESSOR
    and (training, optional) DATA_AUGMENTOR; DATA_PATH when root_path is None."""

    def __init__(self, dataset_cfg, class_names, training=True, root_path=None, logger=None, device="cuda:0"):
        self.dataset_cfg = dataset_cfg
        self.class_names = class_names
        self.training = training
        self.logger = logger
        self.device = device
        self.mode = 'train' if training else 'test'
        self.root_path = Path(root_path if root_path is not None else _get(dataset_cfg, 'DATA_PATH'))
        self.root_split_path = self.root_path
        self.kitti_infos = []
        self._augmentor = self._processor = None
        # `batches` with a transform_points_to_voxels entry: True hands the model `voxel_features` (the voxel means, what
        # MeanVFE -> a sparse backbone reads) in place of the (V, T, C) block `voxels`
        self.voxel_features_only = False
        self.set_split(_get(_get(dataset_cfg, 'DATA_SPLIT'), self.mode))
        self.include_kitti_data(self.mode)

    # ---- the reference's surface ----
    def include_kitti_data(self, mode):
        if self.logger is not None:
            self.logger.info('Loading KITTI dataset')
        kitti_infos = []
        for info_path in _get(_get(self.dataset_cfg, 'INFO_PATH'), mode):
            info_path = self.root_path / info_path
            if not info_path.exists():
                continue
            with open(info_path, 'rb') as f:
                kitti_infos.extend(pickle.load(f))
        self.kitti_infos.extend(kitti_infos)
        if self.logger is not None:
            self.logger.info('Total samples for KITTI dataset: %d' % (len(kitti_infos)))

    def set_split(self, split):
        self.split = split
        split_file = self.root_path / 'ImageSets' / (self.split + '.txt')
        self.sample_id_list = [x.strip() for x in open(split_file).readlines()] if split_file.exists() else None

    def _file(self, folder, idx, ext):
        path = self.root_split_path / folder / ('%s.%s' % (idx, ext))
        if not path.exists():
            raise FileNotFoundError(str(path))
        return path

    def get_lidar(self, idx):
        return np.fromfile(str(self._file('velodyne', idx, 'bin')), dtype=np.float32).reshape(-1, 4)

    def get_calib(self, idx):
        return Calibration(str(self._file('calib', idx, 'txt')))

    def get_label(self, idx):
        return read_label_file(str(self._file('label_2', idx, 'txt')))

    def get_image_shape(self, idx):
        """(h, w) int32 from the PNG's header; without the file, from the infos."""
        path = self.root_split_path / 'image_2' / ('%s.png' % idx)
        if path.exists():
            from PIL import Image
            with Image.open(str(path)) as im:
                w, h = im.size
            return np.array([h, w], dtype=np.int32)
        for info in self.kitti_infos:
            if info['point_cloud']['lidar_idx'] == idx:
                return np.asarray(info['image']['image_shape'], dtype=np.int32)
        raise FileNotFoundError("%s, and no info of frame %s" % (path, idx))

    def get_road_plane(self, idx):
        path = self.root_split_path / 'planes' / ('%s.txt' % idx)
        if not path.exists():
            return None
        with open(path) as f:
            plane = np.asarray([float(v) for v in f.readlines()[3].split()])
        if plane[1] > 0:                                    # the normal points up in the rectified camera frame
            plane = -plane
        return plane / np.linalg.norm(plane[0:3])

    @staticmethod
    def get_fov_flag(pts_rect, img_shape, calib):
        """The reference's host form (:140-156), for its callers; the dataset itself cuts on the GPU."""
        with np.errstate(all="ignore"):
            pts_img, depth = calib.rect_to_img(pts_rect)
            inside = (pts_img[:, 0] >= 0) & (pts_img[:, 0] < img_shape[1]) & (pts_img[:, 1] >= 0) & (pts_img[:, 1] < img_shape[0])
            return inside & (depth >= 0)

    def _count_inside(self, frames, batch_frames=16):
        """frames: (sample id, image shape, (m, 7) float64 boxes) -> per frame the int32 (m) numbers of FOV points inside
        each box: `batch_frames` frames per fov_ingest (DFU3D_ING_COUNT), one host read per batch."""
        import torch
        from .. import ingest_ops
        from .data_augmentor import _h2d
        out = []
        for b0 in range(0, len(frames), batch_frames):
            part = frames[b0:b0 + batch_frames]
            pts = [self.get_lidar(sid) for sid, _, _ in part]
            nb = np.array([len(b) for _, _, b in part], np.int64)
            if nb.sum() == 0:
                out += [np.zeros(0, np.int32) for _ in part]
                continue
            dev = self.device
            r = ingest_ops.fov_ingest(
                _h2d(np.concatenate(pts, 0), dev), _h2d(np.concatenate([[0], np.cumsum([len(p) for p in pts])]).astype(np.int64), dev),
                _h2d(np.stack([self.get_calib(sid).record() for sid, _, _ in part]), dev),
                _h2d(np.stack([np.asarray(s, np.int32).reshape(2) for _, s, _ in part]), dev),
                boxes=_h2d(np.concatenate([np.asarray(b, np.float64).reshape(-1, 7) for _, _, b in part], 0), dev),
                box_off=_h2d(np.concatenate([[0], np.cumsum(nb)]).astype(np.int32), dev), mode=ingest_ops.COUNT)
            host = torch.cat([r.box_cnt, r.status]).cpu().numpy()                  # the one read
            if host[-1]:
                raise Dfu3dError("get_infos: fov_ingest status %d (%s)" % (host[-1], ingest_ops.status_message(int(host[-1]))))
            out += np.split(host[:-1].astype(np.int32), np.cumsum(nb)[:-1])
        return out

    def get_infos(self, num_workers=4, has_label=True, count_inside_pts=True, sample_id_list=None):
        """kitti_dataset.py:158-282.  The host part frame by frame in `num_workers` threads; `num_points_in_gt` for all
        frames together through fov_ingest (no loop over boxes); DontCare rows get -1."""
        def process_single_scene(sample_idx):
            info = {'point_cloud': {'num_features': 4, 'lidar_idx': sample_idx},
                    'image': {'image_idx': sample_idx, 'image_shape': self.get_image_shape(sample_idx)}}
            calib = self.get_calib(sample_idx)
            P2 = np.concatenate([calib.P2, np.array([[0., 0., 0., 1.]])], axis=0)
            R0_4x4 = np.zeros([4, 4], dtype=calib.R0.dtype)
            R0_4x4[3, 3] = 1.
            R0_4x4[:3, :3] = calib.R0
            V2C_4x4 = np.concatenate([calib.V2C, np.array([[0., 0., 0., 1.]])], axis=0)
            info['calib'] = {'P2': P2, 'R0_rect': R0_4x4, 'Tr_velo_to_cam': V2C_4x4}
            if has_label:
                info['annos'] = annotations_of(self.get_label(sample_idx), calib)
            return info

        sample_id_list = sample_id_list if sample_id_list is not None else self.sample_id_list
        with ThreadPoolExecutor(num_workers) as executor:
            infos = list(executor.map(process_single_scene, sample_id_list))
        if has_label and count_inside_pts:
            counts = self._count_inside([(i['point_cloud']['lidar_idx'], i['image']['image_shape'],
                                          i['annos']['gt_boxes_lidar']) for i in infos])
            for info, cnt in zip(infos, counts):
                num = -np.ones(len(info['annos']['name']), dtype=np.int32)
                num[:len(cnt)] = cnt
                info['annos']['num_points_in_gt'] = num
        return infos

    @staticmethod
    def generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=None):
        return generate_prediction_dicts(batch_dict, pred_dicts, class_names, output_path=output_path)

    def evaluation(self, det_annos, class_names, **kwargs):
        if not self.kitti_infos or 'annos' not in self.kitti_infos[0].keys():
            return None, {}
        return evaluation(det_annos, class_names, [info['annos'] for info in self.kitti_infos])

    def __len__(self):
        return len(self.kitti_infos)

    # ---- one frame ----
    def _item_list(self):
        items = list(_get(self.dataset_cfg, 'GET_ITEM_LIST', ['points']))
        for entry in items:
            if entry != 'points':
                raise NotImplementedError("KittiDataset: the GET_ITEM_LIST entry %r is not supported" % (entry,))
        return items

    def _frame(self, index):
        """The host part of __getitem__: (input dict without points, raw points or None)."""
        info = copy.deepcopy(self.kitti_infos[index])
        sample_idx = info['point_cloud']['lidar_idx']
        calib = self.get_calib(sample_idx)
        items = self._item_list()
        d = {'frame_id': sample_idx, 'calib': calib}
        if 'annos' in info:
            annos = drop_info_with_name(info['annos'], name='DontCare')
            loc, dims, rots = annos['location'], annos['dimensions'], annos['rotation_y']
            cam = np.concatenate([loc, dims, rots[..., np.newaxis]], axis=1).astype(np.float32)
            d['gt_names'] = annos['name']
            d['gt_boxes'] = box_utils.boxes3d_kitti_camera_to_lidar(cam, calib)
            road_plane = self.get_road_plane(sample_idx)
            if road_plane is not None:
                d['road_plane'] = road_plane
        d['image_shape'] = info['image']['image_shape']
        return d, (self.get_lidar(sample_idx) if 'points' in items else None)

    def _ingest(self, raw, frames):
        """raw: the frames' (n, 4) arrays; frames: their dicts -> FovIngest over one upload."""
        from .. import ingest_ops
        from .data_augmentor import _h2d
        dev = self.device
        return ingest_ops.fov_ingest(
            _h2d(np.concatenate(raw, 0), dev), _h2d(np.concatenate([[0], np.cumsum([len(p) for p in raw])]).astype(np.int64), dev),
            _h2d(np.stack([d['calib'].record() for d in frames]), dev),
            _h2d(np.stack([np.asarray(d['image_shape'], np.int32).reshape(2) for d in frames]), dev), mode=ingest_ops.EMIT)

    def __getitem__(self, index):
        """The reference's per-frame dict after prepare_data's class selection (dataset.py:194-200): frame_id, calib,
        gt_names and gt_boxes (k, 8: the class id last) of the classes in class_names, the FOV-cut points, image_shape."""
        from .data_augmentor import select_classes
        d, points = self._frame(index)
        if points is not None:
            if _get(self.dataset_cfg, 'FOV_POINTS_ONLY'):
                r = self._ingest([points], [d])
                n = int(r.out_off[1].item())
                points = r.points[:n].cpu().numpy()
            d['points'] = points
        if 'gt_boxes' in d:
            d = select_classes(d, self.class_names)
        return d

    # ---- many frames ----
    @property
    def point_feature_encoder(self):
        enc = _get(self.dataset_cfg, 'POINT_FEATURE_ENCODING', None)
        if enc is None:
            return _Encoder(4)
        used, src = list(_get(enc, 'used_feature_list')), list(_get(enc, 'src_feature_list'))
        cut = self._samples() and 3 <= len(used) < 4 and used == src[:len(used)]      # sample_points copies a prefix
        if len(src) != 4 or not (used == src or cut):
            raise NotImplementedError("KittiDataset: POINT_FEATURE_ENCODING must keep the four columns of the file as they "
                                      "are (or, with a sample_points entry, their first three)")
        return _Encoder(len(used))

    def _samples(self):
        """The DATA_PROCESSOR has a sample_points entry that samples in this mode."""
        for entry in _get(self.dataset_cfg, 'DATA_PROCESSOR', None) or []:
            if _get(entry, 'NAME') == 'sample_points':
                num = _get(entry, 'NUM_POINTS', None)
                return num is not None and _get(num, self.mode) != -1
        return False

    @property
    def point_cloud_range(self):
        return np.array(_get(self.dataset_cfg, 'POINT_CLOUD_RANGE'), dtype=np.float32)

    @property
    def data_processor(self):
        if self._processor is None:
            from .data_processor import DataProcessor
            self._processor = DataProcessor(_get(self.dataset_cfg, 'DATA_PROCESSOR'), self.point_cloud_range, self.training,
                                            self.point_feature_encoder.num_point_features, device=self.device)
        return self._processor

    @property
    def data_augmentor(self):
        """DatasetTemplate's: the DATA_AUGMENTOR of the configuration in training, else (or without the entry) None."""
        cfg = _get(self.dataset_cfg, 'DATA_AUGMENTOR', None)
        if not self.training or cfg is None:
            return None
        if self._augmentor is None:
            from .data_augmentor import DataAugmentor
            self._augmentor = DataAugmentor(self.root_path, cfg, self.class_names, logger=self.logger, device=self.device)
        return self._augmentor

    @property
    def grid_size(self):
        return self.data_processor.grid_size

    @property
    def voxel_size(self):
        return self.data_processor.voxel_size

    def batches(self, batch_size, shuffle=False, seed=0, drop_last=False):
        """A sized iterable of model batch_dicts over the whole dataset; `.dataset` is this object.  shuffle: the frame
        order of every pass is a permutation drawn from numpy.random.default_rng(seed + pass), not from the global RNG the
        augmentor draws from."""
        return Batches(self, batch_size, shuffle, seed, drop_last)

    def collate(self, indices):
        """The frames `indices` as one batch_dict on the device."""
        from .data_augmentor import prepare_batch
        frames, raw = zip(*[self._frame(i) for i in indices])
        if any(p is None for p in raw):
            raise Dfu3dError("KittiDataset.batches: GET_ITEM_LIST has no 'points'")
        B = len(frames)
        if _get(self.dataset_cfg, 'FOV_POINTS_ONLY'):
            r = self._ingest(list(raw), frames)
            off = r.out_off.cpu().numpy()                                          # the one read: the B kept counts
            scenes = [r.points[int(off[b]):int(off[b + 1])] for b in range(B)]
        else:
            scenes = list(raw)
        has_boxes = all('gt_boxes' in d for d in frames)
        dicts = [{'points': p, 'gt_boxes': d['gt_boxes'] if has_boxes else np.zeros((0, 7), np.float32),
                  'gt_names': d['gt_names'] if has_boxes else np.zeros(0, '<U1')} for p, d in zip(scenes, frames)]
        if self.training and has_boxes and self.data_augmentor is not None and self.data_augmentor.sampler is not None:
            for x in dicts:
                x['gt_boxes_mask'] = np.ones(len(x['gt_boxes']), dtype=np.bool_)
        batch = prepare_batch(dicts, self.data_augmentor, self.data_processor, self.class_names, training=self.training,
                              voxel_features_only=self.voxel_features_only)
        if not has_boxes:
            for k in ('gt_boxes', 'gt_cnt', 'empty_scenes'):
                batch.pop(k, None)
        batch['frame_id'] = [d['frame_id'] for d in frames]
        batch['calib'] = [d['calib'] for d in frames]
        batch['image_shape'] = [d['image_shape'] for d in frames]
        return batch


class Batches(object):
    def __init__(self, dataset, batch_size, shuffle=False, seed=0, drop_last=False):
        if batch_size < 1:
            raise Dfu3dError("KittiDataset.batches: batch_size %r" % (batch_size,))
        self.dataset, self.batch_size, self.shuffle, self.seed, self.drop_last = dataset, batch_size, shuffle, seed, drop_last
        self.passes = 0

    def __len__(self):
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        n = len(self.dataset)
        order = np.random.default_rng(self.seed + self.passes).permutation(n) if self.shuffle else np.arange(n)
        self.passes += 1
        for k in range(len(self)):
            yield self.dataset.collate([int(i) for i in order[k * self.batch_size:(k + 1) * self.batch_size]])


def create_kitti_infos(dataset_cfg, class_names, data_path, save_path, workers=4):
    """kitti_dataset.py:504-553 with save_path honoured: kitti_infos_<train split>.pkl, kitti_infos_<val split>.pkl,
    kitti_infos_trainval.pkl under save_path, from the splits DATA_SPLIT names ('train' and 'test'); a split without an
    ImageSets file is left out.  -> {file name: infos}."""
    dataset = KittiDataset(dataset_cfg=dataset_cfg, class_names=class_names, root_path=data_path, training=False)
    splits = _get(dataset_cfg, 'DATA_SPLIT')
    train_split, val_split = _get(splits, 'train'), _get(splits, 'test')
    save_path = Path(save_path)
    save_path.mkdir(parents=True, exist_ok=True)
    written = {}
    for split in dict.fromkeys([train_split, val_split]):
        dataset.set_split(split)
        if dataset.sample_id_list is None:
            continue
        infos = dataset.get_infos(num_workers=workers, has_label=True, count_inside_pts=True)
        written['kitti_infos_%s.pkl' % split] = infos
    if len(written) == 2:
        written['kitti_infos_trainval.pkl'] = written['kitti_infos_%s.pkl' % train_split] + written['kitti_infos_%s.pkl' % val_split]
    for name, infos in written.items():
        with open(save_path / name, 'wb') as f:
            pickle.dump(infos, f)
    return written
