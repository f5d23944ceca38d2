"""Synthetic KITTI frames shared by tests/golden/capture_ingest_golden.py and the ingest / KittiDataset tests: frame
generation, the KITTI directory writer and the reader of golden G18."""
import os

import numpy as np

from dfu3d_amd import kitti_io
from tests import ingest_ref as R

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g18_ingest.npz")
CLASSES = ['Car', 'Pedestrian', 'Bicycle']          # names the KITTI evaluation of this package knows (eval.CLASS_NAMES)
SIZES = {'Car': (3.9, 1.6, 1.5), 'Pedestrian': (0.8, 0.7, 1.75), 'Bicycle': (1.8, 0.6, 1.7), 'Van': (5.0, 1.9, 2.2)}
SHAPES = [(375, 1242), (900, 1600)]
# a point closer than this to a face of a labelled box (x, y faces; z faces) is taken out of a frame: inside that band the
# hull test of the reference and the box rule of csrc/pt_in_box.hpp (1 cm margin in x and y) may differ
BAND_XY, BAND_Z = 0.02, 1e-3
INFO_KEYS = ('name', 'truncated', 'occluded', 'alpha', 'bbox', 'dimensions', 'location', 'rotation_y', 'score',
             'difficulty', 'index', 'gt_boxes_lidar', 'num_points_in_gt')


def face_distance(points, boxes):
    """float64 (m, n, 2): how far every point is from the nearest x / y face plane and from the nearest z face plane of
    every box (x, y, z, dx, dy, dz, heading), in the box's own frame."""
    p = np.asarray(points, np.float64)[None, :, :3] - np.asarray(boxes, np.float64)[:, None, :3]
    b = np.asarray(boxes, np.float64)
    c, s = np.cos(-b[:, 6])[:, None], np.sin(-b[:, 6])[:, None]
    lx, ly = p[..., 0] * c - p[..., 1] * s, p[..., 0] * s + p[..., 1] * c
    dxy = np.minimum(np.abs(np.abs(lx) - b[:, None, 3] / 2), np.abs(np.abs(ly) - b[:, None, 4] / 2))
    return np.stack([dxy, np.abs(np.abs(p[..., 2]) - b[:, None, 5] / 2)], -1)


def label_row(name, box_lidar, calib, bbox=(100.0, 120.0, 260.0, 230.0), trunc=0.0, occ=0):
    """A LiDAR box as the 15 fields of a KITTI label row (two decimals, as KITTI's own files have)."""
    x, y, z, dx, dy, dz, h = box_lidar
    loc = calib.lidar_to_rect(np.array([[x, y, z - dz / 2]], np.float32))[0]
    ry = -h - np.pi / 2
    return '%s %.2f %d %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f %.2f' % (
        name, trunc, occ, -1.5, bbox[0], bbox[1], bbox[2], bbox[3], dz, dy, dx, loc[0], loc[1], loc[2], ry)


def make_frame(frame_id, seed, n, shape, names, yaw=0.0, dontcare=False, fu=720.0):
    """One frame: `n` scattered points plus 60 inside every labelled box, the boxes in front of the camera, the label rows
    (a DontCare row last if asked), points in the face bands removed.  names empty: an empty label file."""
    from dfu3d_amd.labels import LabelObject
    from dfu3d_amd.pcdet_kitti.gt_database import annotations_from_label
    rng = np.random.default_rng(seed)
    calib = R.synthetic_calib(fu=fu, fv=fu, cu=shape[1] / 2 - 0.5, cv=shape[0] / 2 - 0.5, yaw=yaw)
    pts = np.stack([rng.uniform(-10, 40, n), rng.uniform(-20, 20, n), rng.uniform(-2.5, 1.0, n), rng.random(n)], 1)
    rows = []
    for k, name in enumerate(names):
        dx, dy, dz = SIZES[name]
        box = [6.0 + 5.0 * k + rng.uniform(0, 2), rng.uniform(-2.0, 2.0) * (1 + k % 3), -1.0 + rng.uniform(-0.2, 0.2),
               dx, dy, dz, rng.uniform(-np.pi, np.pi)]
        rows.append(label_row(name, box, calib, trunc=0.1 * (k % 3), occ=k % 2,
                              bbox=(50.0 + 90 * k, 100.0, 130.0 + 90 * k, 160.0 + 20 * (k % 3))))
    if dontcare:
        rows.append('DontCare -1 -1 -10 503.89 169.71 590.61 190.13 -1 -1 -1 -1000 -1000 -1000 -10')
    label = "".join(r + "\n" for r in rows)
    ann = annotations_from_label([LabelObject(r) for r in rows], calib)
    boxes = ann['gt_boxes_lidar']
    for b in boxes:                                     # dense inside, in the box's own frame
        l = rng.uniform(-0.45, 0.45, (60, 3)) * b[3:6]
        c, s = np.cos(b[6]), np.sin(b[6])
        inside = np.stack([b[0] + l[:, 0] * c - l[:, 1] * s, b[1] + l[:, 0] * s + l[:, 1] * c, b[2] + l[:, 2],
                           rng.random(60)], 1)
        pts = np.concatenate([pts, inside], 0)
    pts = pts[rng.permutation(len(pts))].astype(np.float32)
    if len(boxes):
        d = face_distance(pts, boxes)
        pts = pts[~((d[..., 0] < BAND_XY) | (d[..., 1] < BAND_Z)).any(0)]
    return {'id': frame_id, 'points': np.ascontiguousarray(pts), 'P2': calib.P2, 'R0': calib.R0, 'V2C': calib.V2C,
            'shape': np.array(shape, np.int32), 'label': label}


def golden_specs():
    """The three frames of G18: a DontCare row; an empty label file; the other image shape and a turned camera."""
    return [dict(frame_id='000000', seed=1801, n=1400, shape=SHAPES[0], names=['Car', 'Pedestrian', 'Bicycle', 'Car', 'Van'],
                 dontcare=True),
            dict(frame_id='000001', seed=1802, n=1500, shape=SHAPES[0], names=[], yaw=0.05),
            dict(frame_id='000002', seed=1803, n=1600, shape=SHAPES[1], names=['Pedestrian', 'Car', 'Bicycle', 'Car'],
                 yaw=-0.1, fu=1260.0)]


def extra_specs():
    """Three more frames for the dataset test: about 2 000 points, 3 to 8 labelled boxes."""
    return [dict(frame_id='000003', seed=1811, n=1800, shape=SHAPES[1], names=['Car', 'Car', 'Pedestrian'], fu=1260.0),
            dict(frame_id='000004', seed=1812, n=1600, shape=SHAPES[0],
                 names=['Car', 'Pedestrian', 'Bicycle', 'Car', 'Pedestrian', 'Car', 'Bicycle', 'Van'], yaw=0.02),
            dict(frame_id='000005', seed=1813, n=1900, shape=SHAPES[0], names=['Bicycle', 'Car', 'Pedestrian', 'Car', 'Car'],
                 yaw=-0.03)]


def calib_of(frame):
    from dfu3d_amd.calibration import Calibration
    return Calibration({'P2': frame['P2'], 'R0': frame['R0'], 'Tr_velo2cam': frame['V2C']})


def write_kitti(root, frames, split='train', images=True):
    """The frames as a KITTI directory: velodyne/ calib/ label_2/ image_2/ (black PNGs of the frame's shape) and
    ImageSets/<split>.txt."""
    from PIL import Image
    root = str(root)
    for d in ('velodyne', 'calib', 'label_2', 'image_2', 'ImageSets'):
        os.makedirs(os.path.join(root, d), exist_ok=True)
    for f in frames:
        f['points'].tofile(os.path.join(root, 'velodyne', f['id'] + '.bin'))
        kitti_io.write_calib(os.path.join(root, 'calib', f['id'] + '.txt'), f['P2'], f['R0'], f['V2C'])
        with open(os.path.join(root, 'label_2', f['id'] + '.txt'), 'w') as fh:
            fh.write(f['label'])
        if images:
            Image.new('L', (int(f['shape'][1]), int(f['shape'][0]))).save(os.path.join(root, 'image_2', f['id'] + '.png'))
    with open(os.path.join(root, 'ImageSets', split + '.txt'), 'w') as fh:
        fh.write("".join(f['id'] + "\n" for f in frames))
    return root


def golden():
    with np.load(PATH) as z:
        return {k: z[k] for k in z.files}


def golden_frames(G=None):
    """The frames of G18 as make_frame returns them, from the recorded arrays."""
    G = G or golden()
    out = []
    for i in range(int(G['n_frames'])):
        p = 'f%d_' % i
        out.append({'id': bytes(G[p + 'id']).decode(), 'points': G[p + 'points'], 'P2': G[p + 'P2'], 'R0': G[p + 'R0'],
                    'V2C': G[p + 'V2C'], 'shape': G[p + 'shape'], 'label': bytes(G[p + 'label']).decode()})
    return out


def all_frames():
    """The six frames of the dataset test: G18's three, then three more."""
    return golden_frames() + [make_frame(**s) for s in extra_specs()]
