"""Row f-10: OpenPCDet's DataAugmentor -- `gt_sampling` (database_sampler.DataBaseSampler) and the four world
entries `random_world_flip`, `random_world_rotation`, `random_world_scaling`, `random_world_translation` -- and the
batched form `prepare_batch` that takes B scenes from the sampler's device output to the model's batch_dict without
leaving device memory (dfu3d_world_aug_collate, include/dfu3d_aug.h).

Reference: pcdet/datasets/augmentor/data_augmentor.py (`__init__` :11-25, the world entries :56-156, `forward`
:290-319), augmentor_utils.py:8-92, common_utils.py (`limit_period`, `rotate_points_along_z`), dataset.py:179-250
(`prepare_data`, `collate_batch`).

The values are drawn on the host from NumPy's global RNG, call for call as the reference's functions draw them for one
scene; everything else runs on the GPU.  Use it in the main process, never inside DataLoader workers.

Divergences from the reference: every entry other than the five above raises
NotImplementedError at construction; the world entries must come in the order flip, rotation, scaling, translation
(each at most once, `gt_sampling` before them); a WORLD_SCALE_RANGE narrower than 1e-3 draws nothing, changes nothing and
writes no `noise_scale` key (the reference's random_world_scaling fails to unpack there); the rotation is one defined
float32 chain; `prepare_batch` neither shuffles nor resamples an empty scene, and draws scene by scene after the
sampler's batch draw.
"""
import numpy as np
import torch

from .. import hard_voxel_ops
from .. import point_sample_ops
from .. import stages as st
from .._lib import Dfu3dError
from .database_sampler import DataBaseSampler

WORLD_ENTRIES = ('random_world_flip', 'random_world_rotation', 'random_world_scaling', 'random_world_translation')


def _cos_sin_f32(noise_rot):
    # rotate_points_along_z: the angle as a float64 array cast to float32, torch's float32 cos / sin
    a = torch.from_numpy(np.array([noise_rot])).float()
    return float(torch.cos(a)[0]), float(torch.sin(a)[0])


def params_record(drawn):
    """The drawn values of one scene (draw_world_params) -> the fields of its dfu3d_aug_params."""
    rec = {'flags': st.AUG_WRAP}
    flips = drawn.get('flips', [])
    for axis, on in flips:
        if on:
            rec['flags'] |= st.AUG_FLIP_X if axis == 'x' else st.AUG_FLIP_Y
    if [a for a, _ in flips] == ['y', 'x']:
        rec['flags'] |= st.AUG_FLIP_Y_FIRST
    if drawn.get('noise_rot') is not None:
        rot = float(drawn['noise_rot'])
        rec['flags'] |= st.AUG_ROTATE
        rec['cos_a'], rec['sin_a'] = _cos_sin_f32(rot)
        rec['noise_rot'], rec['noise_rot_f'] = rot, float(np.float32(rot))
    if drawn.get('noise_scale') is not None:
        sc = float(drawn['noise_scale'])
        rec['flags'] |= st.AUG_SCALE
        rec['scale'], rec['scale_f'] = sc, float(np.float32(sc))
    if drawn.get('noise_translate') is not None:
        t = np.asarray(drawn['noise_translate'], np.float32).reshape(3)
        rec['flags'] |= st.AUG_TRANSLATE
        rec['tx'], rec['ty'], rec['tz'] = float(t[0]), float(t[1]), float(t[2])
    return rec


def class_ids(names, class_names):
    """1-based index into class_names, 0 for a name that is not there (int32)."""
    class_names = list(class_names)
    return np.array([class_names.index(n) + 1 if n in class_names else 0 for n in names], np.int32)


def _on_device(points):
    """A scene's points handed in as a tensor on the GPU (the batched FOV ingest's output) rather than as NumPy."""
    return isinstance(points, torch.Tensor) and points.is_cuda


def _check_scene(points, boxes, what):
    if _on_device(points):
        if points.dim() != 2 or points.dtype != torch.float32 or points.shape[1] < 3:
            raise Dfu3dError("%s: points on the device must be (n, C >= 3) float32" % what)
    elif not isinstance(points, np.ndarray) or points.ndim != 2 or points.dtype != np.float32 or points.shape[1] < 3:
        raise Dfu3dError("%s: points must be (n, C >= 3) float32" % what)
    if not isinstance(boxes, np.ndarray) or boxes.ndim != 2 or boxes.shape[1] not in (7, 9):
        raise Dfu3dError("%s: gt_boxes must be (N, 7) or (N, 9), got %s" % (what, getattr(boxes, 'shape', None)))
    if boxes.dtype not in (np.float32, np.float64):
        raise Dfu3dError("%s: gt_boxes must be float32 or float64" % what)


def _h2d(a, device):
    # through pinned memory and without blocking: an upload is no reason for the host to wait for the device
    t = torch.from_numpy(np.ascontiguousarray(a))
    if torch.device(device).type != 'cuda' or t.numel() == 0:
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


class DataAugmentor(object):
    """Drop-in for pcdet.datasets.augmentor.data_augmentor.DataAugmentor.  `forward(data_dict)`: one scene, NumPy in
    and out, the reference's keys; `prepare_batch(...)` (below): many scenes in one launch chain."""

    def __init__(self, root_path, augmentor_configs, class_names, logger=None, device="cuda:0"):
        self.root_path = root_path
        self.class_names = class_names
        self.logger = logger
        self.device = torch.device(device)
        self.sampler = None
        self.world = {}                      # entry name -> its config, for the entries that are on
        self.data_augmentor_queue = []       # the names, in order
        is_list = isinstance(augmentor_configs, list)
        aug_config_list = augmentor_configs if is_list else augmentor_configs['AUG_CONFIG_LIST']
        disabled = [] if is_list else augmentor_configs.get('DISABLE_AUG_LIST', [])
        for cur_cfg in aug_config_list:
            name = cur_cfg['NAME']
            if name in disabled:
                continue
            if name == 'gt_sampling':
                if self.data_augmentor_queue:
                    raise NotImplementedError("DataAugmentor: gt_sampling must be the first entry")
                self.sampler = self.gt_sampling(config=cur_cfg)
            elif name in WORLD_ENTRIES:
                done = [n for n in self.data_augmentor_queue if n in WORLD_ENTRIES]
                if done and WORLD_ENTRIES.index(done[-1]) >= WORLD_ENTRIES.index(name):
                    raise NotImplementedError("DataAugmentor: the world entries must come in the order %s, each at most "
                                              "once; got %s after %s" % (", ".join(WORLD_ENTRIES), name, done[-1]))
                getattr(self, '_check_' + name)(cur_cfg)
                self.world[name] = cur_cfg
            else:
                raise NotImplementedError("DataAugmentor: the entry %r is not supported" % (name,))
            self.data_augmentor_queue.append(name)

    def gt_sampling(self, config=None):
        return DataBaseSampler(root_path=self.root_path, sampler_cfg=config, class_names=self.class_names,
                               logger=self.logger, device=self.device)

    @staticmethod
    def _check_random_world_flip(cfg):
        axes = list(cfg['ALONG_AXIS_LIST'])
        if any(a not in ('x', 'y') for a in axes) or len(set(axes)) != len(axes):
            raise NotImplementedError("random_world_flip: ALONG_AXIS_LIST must name 'x' and 'y' at most once each")

    @staticmethod
    def _check_random_world_rotation(cfg):
        cfg['WORLD_ROT_ANGLE']

    @staticmethod
    def _check_random_world_scaling(cfg):
        if len(cfg['WORLD_SCALE_RANGE']) != 2:
            raise Dfu3dError("random_world_scaling: WORLD_SCALE_RANGE must be [lo, hi]")

    @staticmethod
    def _check_random_world_translation(cfg):
        if len(cfg['NOISE_TRANSLATE_STD']) != 3:
            raise Dfu3dError("random_world_translation: NOISE_TRANSLATE_STD must have 3 values")

    def draw_world_params(self, n_gt_cols=7):
        """What the reference's world entries draw for one scene, from NumPy's global RNG, in queue order.  n_gt_cols
        (7 or 9) is checked only: no draw depends on it.  -> {'flips': [(axis, np.bool_), ...], 'noise_rot',
        'noise_scale', 'noise_translate'} (None for an entry that is off or draws nothing)."""
        if n_gt_cols not in (7, 9):
            raise Dfu3dError("draw_world_params: boxes of %d columns" % n_gt_cols)
        drawn = {'flips': [], 'noise_rot': None, 'noise_scale': None, 'noise_translate': None}
        if 'random_world_flip' in self.world:
            for axis in self.world['random_world_flip']['ALONG_AXIS_LIST']:
                drawn['flips'].append((axis, np.random.choice([False, True], replace=False, p=[0.5, 0.5])))
        if 'random_world_rotation' in self.world:
            rot_range = self.world['random_world_rotation']['WORLD_ROT_ANGLE']
            if not isinstance(rot_range, list):
                rot_range = [-rot_range, rot_range]
            drawn['noise_rot'] = np.random.uniform(rot_range[0], rot_range[1])
        if 'random_world_scaling' in self.world:
            lo, hi = self.world['random_world_scaling']['WORLD_SCALE_RANGE']
            if not hi - lo < 1e-3:
                drawn['noise_scale'] = np.random.uniform(lo, hi)
        if 'random_world_translation' in self.world:
            std = self.world['random_world_translation']['NOISE_TRANSLATE_STD']
            drawn['noise_translate'] = np.array([np.random.normal(0, std[0], 1), np.random.normal(0, std[1], 1),
                                                 np.random.normal(0, std[2], 1)], dtype=np.float32).T
        return drawn

    def forward(self, data_dict):
        """One scene (data_augmentor.py:290-319): points (n, C) float32, gt_boxes (N, 7|9), gt_names, optionally
        gt_boxes_mask and road_plane; updated and returned.  The same kernels as the batched form, at B = 1."""
        if self.sampler is not None:
            data_dict = self.sampler(data_dict)
        points, boxes = data_dict['points'], data_dict['gt_boxes']
        _check_scene(points, boxes, "DataAugmentor.forward")
        drawn = self.draw_world_params(boxes.shape[1])
        n, m = points.shape[0], boxes.shape[0]
        dev = self.device
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        out, _, _, _, _, aug, _ = st.world_aug_collate(
            _h2d(points, dev), _h2d(np.array([0, n], np.int64), dev), _h2d(boxes, dev),
            _h2d(np.array([0, m], np.int32), dev), _h2d(np.array([m], np.int32), dev),
            torch.ones(m, dtype=torch.int32, device=dev), _h2d(st.aug_params([params_record(drawn)]), dev),
            torch.zeros(6, dtype=torch.float32, device=dev), 0, m, status, want_aug=True)
        word = int(status.item())
        if word:
            raise Dfu3dError("DataAugmentor.forward: status %d (%s)" % (word, st.aug_status_message(word)))
        data_dict['points'] = out[:, 1:].cpu().numpy()
        data_dict['gt_boxes'] = aug.cpu().numpy()
        for axis, on in drawn['flips']:
            data_dict['flip_%s' % axis] = on
        for key in ('noise_rot', 'noise_scale', 'noise_translate'):
            name = 'random_world_' + {'noise_rot': 'rotation', 'noise_scale': 'scaling',
                                      'noise_translate': 'translation'}[key]
            if name in self.world and drawn[key] is not None:
                data_dict[key] = drawn[key]
        if 'road_plane' in data_dict:
            data_dict.pop('road_plane')
        if 'gt_boxes_mask' in data_dict:
            gt_boxes_mask = data_dict['gt_boxes_mask']
            data_dict['gt_boxes'] = data_dict['gt_boxes'][gt_boxes_mask]
            data_dict['gt_names'] = data_dict['gt_names'][gt_boxes_mask]
            if 'gt_boxes2d' in data_dict:
                data_dict['gt_boxes2d'] = data_dict['gt_boxes2d'][gt_boxes_mask]
            data_dict.pop('gt_boxes_mask')
        return data_dict


def select_classes(data_dict, class_names):
    """dataset.py:194-200 for one scene on the host: the boxes whose name is in class_names, with `index + 1` appended as
    a float32 column."""
    names = np.asarray(data_dict['gt_names'])
    cls = class_ids(names, class_names)
    sel = cls > 0
    data_dict['gt_boxes'] = np.concatenate((data_dict['gt_boxes'][sel], cls[sel].reshape(-1, 1).astype(np.float32)),
                                           axis=1)
    data_dict['gt_names'] = names[sel]
    return data_dict


def _pack_host(data_dicts, class_names, device):
    """Scenes that did not come through the sampler -> the stage's device operands."""
    pts, boxes, cls = [], [], []
    for d in data_dicts:
        p, b = d['points'], d['gt_boxes']
        _check_scene(p, b, "prepare_batch")
        c = class_ids(d['gt_names'], class_names)
        if len(c) != len(b):
            raise Dfu3dError("prepare_batch: %d names for %d boxes" % (len(c), len(b)))
        if d.get('gt_boxes_mask', None) is not None:
            keep = np.asarray(d['gt_boxes_mask'], bool)
            b, c = b[keep], c[keep]
        pts.append(p)
        boxes.append(b)
        cls.append(c)
    if len({p.shape[1] for p in pts}) > 1 or len({(b.shape[1], b.dtype) for b in boxes}) > 1:
        raise Dfu3dError("prepare_batch: the scenes' point columns, box columns and box dtypes must agree")
    npts = np.array([len(p) for p in pts], np.int64)
    nbox = np.array([len(b) for b in boxes], np.int64)
    if any(_on_device(p) for p in pts):                   # scenes already on the device: concatenated there
        points = torch.cat([p.to(device) if _on_device(p) else _h2d(p, device) for p in pts], 0)
    else:
        points = _h2d(np.concatenate(pts, 0), device)
    return {
        'points': points,
        'point_off': _h2d(np.concatenate([[0], np.cumsum(npts)]).astype(np.int64), device),
        'boxes': _h2d(np.concatenate(boxes, 0), device),
        'box_off': _h2d(np.concatenate([[0], np.cumsum(nbox)]).astype(np.int32), device),
        'box_cnt': _h2d(nbox.astype(np.int32), device), 'box_cls': _h2d(np.concatenate(cls, 0), device),
        'box_cap': int(nbox.max()), 'n_cols': boxes[0].shape[1], 'status': [],
    }


def _pack_sampled(sampler, data_dicts, class_names, device):
    """The sampler's device output (GtSampleBatch) as the stage's operands: nothing comes back to the host."""
    g = sampler.sample_batch(data_dicts)
    dtypes = {np.dtype(sc['dtype']) for sc in g.scenes}
    if len(dtypes) > 1:
        raise Dfu3dError("prepare_batch: the scenes' box dtypes must agree")
    # class id of every INPUT row of the sampler (ground truths, then candidates); its output rows name their input
    # row in box_src, so the ids follow by one gather on the device
    cls_in = np.concatenate([class_ids(list(np.asarray(sc['dict']['gt_names']).astype(str)) + list(sc['cand_names']),
                                       class_names) for sc in g.scenes])
    spans = np.array([sc['boxes'].shape[0] for sc in g.scenes], np.int64)
    base = np.repeat(np.concatenate([[0], np.cumsum(spans)[:-1]]), spans).astype(np.int64)
    cls = _h2d(cls_in, device)[_h2d(base, device) + g.box_src.long()] if len(cls_in) else _h2d(cls_in, device)
    boxes = g.boxes if dtypes == {np.dtype(np.float64)} else g.boxes.float()
    return {
        'points': g.points, 'point_off': g.point_off, 'boxes': boxes.contiguous(), 'box_off': g.box_off,
        'box_cnt': g.box_cnt, 'box_cls': cls.contiguous(), 'box_cap': int(spans.max()), 'n_cols': 7,
        'status': [g.status],
    }


def prepare_batch(data_dicts, augmentor, processor, class_names, training=True, as_padded=False,
                  voxel_features_only=False):
    """B scenes -> the model's batch_dict on the device: `points` (sum n, 1 + C) with the batch index in column 0,
    `gt_boxes` (B, max_gt, 8|10) zero-padded with the class id last, `batch_size`, `gt_cnt` (B).

    data_dicts: NumPy dicts (points, gt_boxes, gt_names[, gt_boxes_mask]); a scene's `points` may also be a float32
    tensor on the GPU (KittiDataset.batches hands the FOV ingest's output over so), concatenated on the device then.
    With a `gt_sampling` entry (and training)
    they go through DataBaseSampler.sample_batch first and stay on the device from there.  One draw per scene
    (augmentor.draw_world_params), then one launch chain.  augmentor None: no augmentation.
    Default: ONE host read (n_kept, the B box counts and the status words together) to cut points[:n_kept] and
    gt_boxes[:, :max(gt_cnt)].  as_padded=True: no host read at all; `points` keeps every input row (rows at or beyond
    `n_kept` carry batch index -1), `gt_boxes` is (B, box_cap, .), and `n_kept`, `point_cnt`, `status` are device tensors.
    A processor with a `sample_points` entry (processor.sample_count()): what the range mask kept of every scene goes
    through point_sample_ops.sample_points, so `points` is (B * K, 1 + processor.num_point_features) in both forms and
    `point_cnt` is K for every scene; a scene the mask left without points raises in the default form (the same one
    read) and sets DFU3D_SMP_EMPTY_SCENE in its word of `status` in the padded form.
    A processor with a `transform_points_to_voxels` entry (processor.voxel_config()): what the mask, and the sampling if
    there is one, left goes through hard_voxel_ops.hard_voxels in the order it arrives; the batch gains `voxels` (V, T, C),
    `voxel_coords` (V, 4) [b, z, y, x], `voxel_num_points` (V) and `voxel_cnt` (B), and `points` stays.  Default form:
    V = n_voxels, which joins the one read, as does the stage's status word (checked last).  Padded form: V = V_cap,
    `n_voxels` is a device tensor and the status word is the last of `status`.  voxel_features_only=True: `voxel_features`
    (V, C), the mean of every voxel's rows (what MeanVFE makes of `voxels`, the same bits), instead of `voxels`."""
    B = len(data_dicts)
    if B == 0:
        raise Dfu3dError("prepare_batch: no scenes")
    device = augmentor.device if augmentor is not None else processor.device
    if augmentor is not None and augmentor.sampler is not None and training:
        u = _pack_sampled(augmentor.sampler, data_dicts, class_names, device)
    else:
        u = _pack_host(data_dicts, class_names, device)
    if augmentor is not None and training:
        recs = [params_record(augmentor.draw_world_params(u['n_cols'])) for _ in range(B)]
    else:
        recs = [{'flags': 0} for _ in range(B)]
    mode = st.AUG_FILTER_CLASS | processor.mask_mode()
    status = torch.zeros(1, dtype=torch.int32, device=device)
    out, n_kept, point_cnt, gt, gt_cnt, _, _ = st.world_aug_collate(
        u['points'], u['point_off'], u['boxes'], u['box_off'], u['box_cnt'], u['box_cls'],
        _h2d(st.aug_params(recs), device), processor.range_tensor(), mode, max(u['box_cap'], 1), status)
    batch = {'batch_size': B, 'gt_cnt': gt_cnt}
    words = [status] + u['status']
    k = processor.sample_count()
    if k is not None:                                      # what the mask kept of every scene -> k rows of it
        if processor.num_point_features > out.shape[1] - 1:
            raise Dfu3dError("prepare_batch: the processor's %d point features, the scenes have %d columns"
                             % (processor.num_point_features, out.shape[1] - 1))
        out, sampled = point_sample_ops.sample_points(out, point_cnt, k, out_cols=processor.num_point_features)
        n_kept = torch.full((1,), B * k, dtype=torch.int32, device=device)
        point_cnt = torch.full((B,), k, dtype=torch.int32, device=device)
        words.append(sampled)
    vc = processor.voxel_config()
    if vc is not None:                                     # what is left of every scene -> its voxels
        cols = min(processor.num_point_features, out.shape[1] - 1)
        hv = hard_voxel_ops.hard_voxels(out, point_cnt, processor.point_cloud_range, vc['voxel_size'], vc['grid_size'],
                                        vc['max_points'], vc['max_voxels'], out_cols=cols,
                                        want_voxels=not voxel_features_only, want_mean=voxel_features_only)
        vox = {'voxel_coords': hv.voxel_coords, 'voxel_num_points': hv.voxel_num_points}
        vox.update({'voxel_features': hv.voxel_mean} if voxel_features_only else {'voxels': hv.voxels})
        batch['voxel_cnt'] = hv.voxel_cnt
    if as_padded:
        batch.update(points=out, gt_boxes=gt, n_kept=n_kept, point_cnt=point_cnt, status=words)
        if vc is not None:
            batch.update(vox, n_voxels=hv.n_voxels, status=words + [hv.status])
        return batch
    tail = [hv.status, hv.n_voxels] if vc is not None else []
    host = torch.cat([n_kept, gt_cnt] + [s.reshape(1) for s in words + tail]).cpu().numpy()             # the one read
    if vc is not None:
        host, (hv_status, n_vox) = host[:-2], (int(host[-2]), int(host[-1]))
    if host[B + 1]:
        raise Dfu3dError("prepare_batch: status %d (%s)" % (host[B + 1], st.aug_status_message(int(host[B + 1]))))
    if u['status'] and host[B + 2]:
        raise Dfu3dError("prepare_batch: gt_sample status %d" % host[B + 2])
    if k is not None and host[-1]:
        raise Dfu3dError("prepare_batch: sample_points status %d (%s)"
                         % (host[-1], point_sample_ops.status_message(int(host[-1]))))
    if vc is not None:
        if hv_status:
            raise Dfu3dError("prepare_batch: transform_points_to_voxels status %d (%s)"
                             % (hv_status, hard_voxel_ops.status_message(hv_status)))
        batch.update({key: t[:n_vox] for key, t in vox.items()})
    batch.update(points=out[:int(host[0])], gt_boxes=gt[:, :int(host[1:B + 1].max())].contiguous(),
                 point_cnt=point_cnt, empty_scenes=[b for b in range(B) if host[1 + b] == 0])
    return batch
