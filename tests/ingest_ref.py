"""NumPy restatement of the batched FOV ingest (include/dfu3d_ingest.h) -- TEST INFRASTRUCTURE ONLY.

The keep flag goes through dfu3d_amd.calibration.Calibration.lidar_to_img, the host form of the float32 chains golden G7
pins to the reference; the gather is NumPy's boolean index (stable); the box count is the rule of csrc/pt_in_box.hpp as
oracle/gtdb_oracle.py states it (float32 differences and rotation, the comparisons in float64), over the kept points."""
import numpy as np

from dfu3d_amd.calibration import Calibration
from oracle.gtdb_oracle import points_in_boxes_cpu


def synthetic_calib(fu=720.0, fv=720.0, cu=620.5, cv=187.0, yaw=0.0, t=(0.0, -0.08, -0.27), tx=-44.0):
    """A KITTI-like calibration: the camera looks along LiDAR +x, turned by `yaw` about LiDAR z."""
    c, s = np.cos(yaw), np.sin(yaw)
    # camera x = -LiDAR y, camera y = -LiDAR z, camera z = LiDAR x, after the turn
    R = np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], np.float64) @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1]], np.float64)
    return Calibration({'P2': np.array([[fu, 0, cu, tx], [0, fv, cv, 0.2], [0, 0, 1, 0.003]], np.float32),
                        'R0': np.eye(3, dtype=np.float32),
                        'Tr_velo2cam': np.concatenate([R, np.array(t, np.float64).reshape(3, 1)], 1).astype(np.float32)})


def fov_flag(points, calib, image_shape):
    """get_fov_flag over lidar_to_rect (kitti_dataset.py:140-156, 483-484): bool (n)."""
    pts = np.asarray(points, np.float32)
    if pts.shape[0] == 0:
        return np.zeros(0, bool)
    with np.errstate(all="ignore"):
        img, depth = calib.lidar_to_img(pts[:, 0:3])
        h, w = np.float32(image_shape[0]), np.float32(image_shape[1])
        return (img[:, 0] >= 0) & (img[:, 0] < w) & (img[:, 1] >= 0) & (img[:, 1] < h) & (depth >= 0)


def box_counts(kept, boxes):
    """int32 (m): kept points inside each (x, y, z, dx, dy, dz, heading) box."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    if boxes.shape[0] == 0 or kept.shape[0] == 0:
        return np.zeros(boxes.shape[0], np.int32)
    with np.errstate(all="ignore"):
        return points_in_boxes_cpu(kept[:, :3], boxes).sum(1).astype(np.int32)


def fov_ingest(scenes, calibs, shapes, boxes=None):
    """scenes: float32 (n_b, C) per frame; calibs: Calibration per frame; shapes: (h, w) per frame; boxes: (m_b, 7) per
    frame or None.  -> (kept rows of all frames (sum k, C), out_off int64 (B + 1), flags per frame, counts int32 (sum m)
    or None)."""
    flags = [fov_flag(p, c, s) for p, c, s in zip(scenes, calibs, shapes)]
    kept = [np.asarray(p, np.float32)[f] for p, f in zip(scenes, flags)]
    off = np.concatenate([[0], np.cumsum([len(k) for k in kept])]).astype(np.int64)
    cnt = None
    if boxes is not None:
        cnt = np.concatenate([box_counts(k, b) for k, b in zip(kept, boxes)] + [np.zeros(0, np.int32)]).astype(np.int32)
    C = scenes[0].shape[1]
    return np.concatenate(kept + [np.zeros((0, C), np.float32)], 0), off, flags, cnt
