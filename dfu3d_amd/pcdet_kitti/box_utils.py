"""The box conversions between a detector's LiDAR boxes and KITTI result rows (pcdet/utils/box_utils.py:203-288), used
by generate_prediction_dicts, and from a label's camera box to the LiDAR frame (:134-150), used by KittiDataset.  Host NumPy on a few hundred boxes per frame, as in the reference; same dtypes (float32
corner offsets, the rotation in the dtype of the boxes)."""
import numpy as np


def boxes3d_lidar_to_kitti_camera(boxes3d_lidar, calib):
    """(N,7) [x y z dx dy dz heading] (centre) -> (N,7) [x y z l h w ry] in the rectified camera frame, y at the box
    bottom (box_utils.py:203-219)."""
    b = np.array(boxes3d_lidar, copy=True)
    xyz = b[:, 0:3]
    l, w, h = b[:, 3:4], b[:, 4:5], b[:, 5:6]
    xyz[:, 2] -= h.reshape(-1) / 2
    xyz_cam = calib.lidar_to_rect(xyz)
    ry = -b[:, 6:7] - np.pi / 2
    return np.concatenate([xyz_cam, l, h, w, ry], axis=-1)


def boxes3d_to_corners3d_kitti_camera(boxes3d, bottom_center=True):
    """(N,7) camera boxes -> (N,8,3) corners, 0-3 the bottom face, 4-7 the top face (box_utils.py:222-265)."""
    n = boxes3d.shape[0]
    l, h, w = boxes3d[:, 3], boxes3d[:, 4], boxes3d[:, 5]
    sx = np.array([1, 1, -1, -1, 1, 1, -1, -1], np.float64) / 2.
    sz = np.array([1, -1, -1, 1, 1, -1, -1, 1], np.float64) / 2.
    x_c = (l[:, None] * sx[None, :]).astype(np.float32)
    z_c = (w[:, None] * sz[None, :]).astype(np.float32)
    if bottom_center:
        y_c = np.zeros((n, 8), np.float32)
        y_c[:, 4:8] = -h.reshape(n, 1).repeat(4, axis=1)
    else:
        y_c = (h[:, None] * np.array([1, 1, 1, 1, -1, -1, -1, -1], np.float64)[None, :] / 2.).astype(np.float32)
    ry = boxes3d[:, 6]
    zeros, ones = np.zeros(ry.size, np.float32), np.ones(ry.size, np.float32)
    R = np.transpose(np.array([[np.cos(ry), zeros, -np.sin(ry)], [zeros, ones, zeros], [np.sin(ry), zeros, np.cos(ry)]]),
                     (2, 0, 1))
    rotated = np.matmul(np.stack([x_c, y_c, z_c], axis=2), R)
    centre = boxes3d[:, 0:3].reshape(-1, 1, 3)
    return np.stack([centre[:, :, 0] + rotated[:, :, 0], centre[:, :, 1] + rotated[:, :, 1],
                     centre[:, :, 2] + rotated[:, :, 2]], axis=2).astype(np.float32)


def boxes3d_kitti_camera_to_imageboxes(boxes3d, calib, image_shape=None):
    """(N,7) camera boxes -> (N,4) [x1 y1 x2 y2]: the bounding rectangle of the eight projected corners, clipped to the
    image when its (height, width) is given (box_utils.py:268-288)."""
    corners = boxes3d_to_corners3d_kitti_camera(boxes3d)
    pts_img, _ = calib.rect_to_img(corners.reshape(-1, 3))
    uv = pts_img.reshape(-1, 8, 2)
    boxes = np.concatenate([np.min(uv, axis=1), np.max(uv, axis=1)], axis=1)
    if image_shape is not None:
        boxes[:, 0::2] = np.clip(boxes[:, 0::2], a_min=0, a_max=image_shape[1] - 1)
        boxes[:, 1::2] = np.clip(boxes[:, 1::2], a_min=0, a_max=image_shape[0] - 1)
    return boxes


def boxes3d_kitti_camera_to_lidar(boxes3d_camera, calib):
    """(N,7) [x y z l h w ry] in the rectified camera frame, y at the box bottom -> (N,7) [x y z dx dy dz heading], the
    centre in the LiDAR frame (box_utils.py:134-150).  The input is not written."""
    b = np.array(boxes3d_camera, copy=True)
    r = b[:, 6:7]
    l, h, w = b[:, 3:4], b[:, 4:5], b[:, 5:6]
    xyz_lidar = calib.rect_to_lidar(b[:, 0:3])
    xyz_lidar[:, 2] += h[:, 0] / 2
    return np.concatenate([xyz_lidar, l, w, h, -(r + np.pi / 2)], axis=-1)


def enlarge_box3d(boxes3d, extra_width=(0, 0, 0)):
    """(N, 7 + C) [x y z dx dy dz heading ...], NumPy or torch -> a copy (torch) with extra_width added to dx, dy, dz in
    the boxes' dtype (box_utils.py:187-200)."""
    import torch
    boxes3d = torch.from_numpy(boxes3d).float() if isinstance(boxes3d, np.ndarray) else boxes3d
    large = boxes3d.clone()
    large[:, 3:6] += boxes3d.new_tensor(extra_width)[None, :]
    return large


def rotate_points_along_z(points, angle):
    """points (B, N, 3 + C), angle (B) about z, x towards y -> the rotated points, the other columns unchanged
    (common_utils.py:35-57): [x', y'] = [x cos - y sin, x sin + y cos]."""
    import torch
    is_numpy = isinstance(points, np.ndarray)
    points = torch.from_numpy(points).float() if is_numpy else points
    angle = torch.from_numpy(angle).float() if isinstance(angle, np.ndarray) else angle
    cosa, sina = torch.cos(angle), torch.sin(angle)
    zeros, ones = angle.new_zeros(points.shape[0]), angle.new_ones(points.shape[0])
    rot = torch.stack((cosa, sina, zeros, -sina, cosa, zeros, zeros, zeros, ones), dim=1).view(-1, 3, 3).float()
    out = torch.cat((torch.matmul(points[:, :, 0:3], rot), points[:, :, 3:]), dim=-1)
    return out.numpy() if is_numpy else out


CORNER_SIGNS = ((1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1))


def boxes_to_corners_3d(boxes3d):
    """(N, 7) [x y z dx dy dz heading] torch -> (N, 8, 3): corners 0-3 the bottom face, 4-7 the top face, each face
    counter-clockwise from (+x, +y) in the box frame as CORNER_SIGNS lists them (box_utils.py:28-53)."""
    half = boxes3d.new_tensor(CORNER_SIGNS) / 2
    corners = boxes3d[:, None, 3:6].repeat(1, 8, 1) * half[None, :, :]
    corners = rotate_points_along_z(corners.view(-1, 8, 3), boxes3d[:, 6]).view(-1, 8, 3)
    return corners + boxes3d[:, None, 0:3]


def boxes_iou_normal(boxes_a, boxes_b):
    """(N, 4), (M, 4) [x1, y1, x2, y2] torch -> (N, M): overlap over clamp_min(union, 1e-6) (box_utils.py:291-311)."""
    import torch
    assert boxes_a.shape[1] == boxes_b.shape[1] == 4
    x_len = torch.clamp_min(torch.min(boxes_a[:, 2, None], boxes_b[None, :, 2])
                            - torch.max(boxes_a[:, 0, None], boxes_b[None, :, 0]), min=0)
    y_len = torch.clamp_min(torch.min(boxes_a[:, 3, None], boxes_b[None, :, 3])
                            - torch.max(boxes_a[:, 1, None], boxes_b[None, :, 1]), min=0)
    area_a = (boxes_a[:, 2] - boxes_a[:, 0]) * (boxes_a[:, 3] - boxes_a[:, 1])
    area_b = (boxes_b[:, 2] - boxes_b[:, 0]) * (boxes_b[:, 3] - boxes_b[:, 1])
    overlap = x_len * y_len
    return overlap / torch.clamp_min(area_a[:, None] + area_b[None, :] - overlap, min=1e-6)


def boxes3d_lidar_to_aligned_bev_boxes(boxes3d):
    """(N, 7 + C) torch -> (N, 4) [x1, y1, x2, y2]: the footprint turned to the nearer axis (box_utils.py:314-325)."""
    import torch
    from .common_utils import limit_period
    turn = limit_period(boxes3d[:, 6], offset=0.5, period=np.pi).abs()
    dims = torch.where(turn[:, None] < np.pi / 4, boxes3d[:, [3, 4]], boxes3d[:, [4, 3]])
    return torch.cat((boxes3d[:, 0:2] - dims / 2, boxes3d[:, 0:2] + dims / 2), dim=1)


def boxes3d_nearest_bev_iou(boxes_a, boxes_b):
    """(N, 7), (M, 7) torch -> (N, M): the IoU of the axis-aligned footprints (box_utils.py:328-340)."""
    return boxes_iou_normal(boxes3d_lidar_to_aligned_bev_boxes(boxes_a), boxes3d_lidar_to_aligned_bev_boxes(boxes_b))
