"""Drop-in for the box geometry of pcdet/models/model_utils/centernet_utils.py: `gaussian_radius` and
`decode_bbox_from_heatmap` with the reference's names, arguments and returns; the decode runs in
csrc/centerhead_stage.hip (dfu3d_center_decode), one launch for the whole batch.

Order of the returned rows: descending score, ties by ascending flat index class * H * W + cell (torch.topk leaves ties
unspecified; an untrained head produces nothing but ties).  NaN ranks above every number, as in torch.topk."""
import torch

from .. import stages
from .._lib import Dfu3dError


def gaussian_radius(height, width, min_overlap=0.5):
    """centernet_utils.py:9-35, tensors in, tensor out (the three roots as written there; r3 is not divided by a3)."""
    b1 = (height + width)
    c1 = width * height * (1 - min_overlap) / (1 + min_overlap)
    r1 = (b1 + (b1 ** 2 - 4 * c1).sqrt()) / 2
    b2 = 2 * (height + width)
    c2 = (1 - min_overlap) * width * height
    r2 = (b2 + (b2 ** 2 - 16 * c2).sqrt()) / 2
    a3 = 4 * min_overlap
    b3 = -2 * min_overlap * (height + width)
    c3 = (min_overlap - 1) * width * height
    r3 = (b3 + (b3 ** 2 - 4 * a3 * c3).sqrt()) / 2
    return torch.min(torch.min(r1, r2), r3)


def _f32(v):
    """The float32 value of a Python / NumPy / tensor scalar, as torch rounds a scalar operand of a float32 tensor."""
    return float(torch.tensor(float(v), dtype=torch.float32))


def decode_raw(heatmap, rot_cos, rot_sin, center, center_z, dim, point_cloud_range, voxel_size, feature_map_stride,
               vel=None, iou=None, K=100, circle_nms=False, score_thresh=None, post_center_limit_range=None, out=None):
    """The kernel's padded result: boxes (B,K,7|9), scores (B,K), labels int32 (B,K), iou (B,K) | None, count int32 (B),
    all on the device and without a host read.  out: the same tuple preallocated (stages.center_decode) to write into."""
    if circle_nms:
        raise NotImplementedError("decode_bbox_from_heatmap: circle_nms is 'not checked yet' in the reference (assert False)")
    if post_center_limit_range is None:
        raise ValueError("decode_bbox_from_heatmap: post_center_limit_range is required")
    if heatmap.dim() != 4:
        raise Dfu3dError("decode_bbox_from_heatmap: heatmap must be (B, n_cls, H, W)")
    B, n_cls, H, W = heatmap.shape
    K = int(K)
    if K < 1 or K > n_cls * H * W:
        raise RuntimeError("decode_bbox_from_heatmap: K = %d is out of range for %d scores per sample" % (K, n_cls * H * W))
    if K > stages.CENTER_MAX_K:
        raise Dfu3dError("decode_bbox_from_heatmap: K = %d, the kernel holds at most %d (DFU3D_ERANGE)"
                         % (K, stages.CENTER_MAX_K))
    if int(feature_map_stride) != feature_map_stride:
        raise Dfu3dError("decode_bbox_from_heatmap: feature_map_stride must be an integer")
    limit = torch.as_tensor(post_center_limit_range, dtype=torch.float32, device=heatmap.device).contiguous()
    c = lambda t: None if t is None else t.float().contiguous()   # noqa: E731
    return stages.center_decode(c(heatmap), c(rot_cos), c(rot_sin), c(center), c(center_z), c(dim), c(vel), c(iou), K,
                                (_f32(point_cloud_range[0]), _f32(point_cloud_range[1])),
                                (_f32(voxel_size[0]), _f32(voxel_size[1])), int(feature_map_stride), limit, score_thresh,
                                out=out)


def decode_bbox_from_heatmap(heatmap, rot_cos, rot_sin, center, center_z, dim,
                             point_cloud_range=None, voxel_size=None, feature_map_stride=None, vel=None, iou=None, K=100,
                             circle_nms=False, score_thresh=None, post_center_limit_range=None):
    """centernet_utils.py:173-241 -> [{'pred_boxes', 'pred_scores', 'pred_labels'[, 'pred_iou']}] per sample.  The only
    host read is the per-sample row counts."""
    boxes, scores, labels, iou_out, count = decode_raw(
        heatmap, rot_cos, rot_sin, center, center_z, dim, point_cloud_range, voxel_size, feature_map_stride, vel=vel,
        iou=iou, K=K, circle_nms=circle_nms, score_thresh=score_thresh, post_center_limit_range=post_center_limit_range)
    ret = []
    for k, n in enumerate(count.tolist()):
        ret.append({'pred_boxes': boxes[k, :n], 'pred_scores': scores[k, :n], 'pred_labels': labels[k, :n]})
        if iou_out is not None:
            ret[-1]['pred_iou'] = iou_out[k, :n]
    return ret
